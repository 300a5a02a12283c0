// Native rescoring session: the moderation rescan of a batch's rewritten rows
// (featurize → classifier GEMM → gemv head → scores on the host) submitted
// by ONE call that allocates nothing, frees nothing and never synchronises.
//
// The session owns, per slot: a pinned host arena [int32 offs (max_rows+1) |
// bytes] and its device mirror (one H2D copy carries spans and text), device
// feats / h / scores, pinned scores and one event. The kernels are the
// library's own forge_featurize, forge_gemm_bt_skinny (or forge_gemm_bt) and
// forge_gemv_head, so the scores are bit-identical to the eager path's. Rows
// are independent in all three, so stale rows of the padding need no fill.
//
// The classifier weights are borrowed device pointers: the caller keeps them
// alive for the session's lifetime.
//
// Threading: a session belongs to ONE thread (the asyncio thread). It is not
// thread-safe. The one exception is forge_rescore_wait, which only blocks on
// the slot's event and may run on a helper thread while the owner does
// nothing else with that slot.

#include "common.h"

#include <stdlib.h>
#include <string.h>

#include <new>

namespace {

enum : int { SLOT_FREE = 0, SLOT_BUSY = 1, SLOT_DRAINING = 2 };

struct RescoreSlot {
    uint8_t* pin_arena = nullptr;   // [int32 offs (max_rows+1) | pad to 16 | bytes]
    uint8_t* dev_arena = nullptr;
    short* feats = nullptr;         // [rows_cap, dim] bf16
    short* h = nullptr;             // [rows_cap, hidden] bf16
    float* scores = nullptr;        // [rows_cap, classes]
    float* pin_scores = nullptr;    // [max_rows, classes]
    hipEvent_t done = nullptr;
    int state = SLOT_FREE;
};

struct RescoreSession {
    const void* w1t; const void* b1; const void* w2t; const void* b2;
    int dim, hidden, classes, max_rows, rows_cap, n_slots;
    int64_t max_bytes, bytes_off;
    bool skinny;
    RescoreSlot* slots;
};

int round_up(int v, int m) { return (v + m - 1) / m * m; }

void free_session(RescoreSession* s) {
    if (s == nullptr) return;
    for (int i = 0; s->slots != nullptr && i < s->n_slots; ++i) {
        RescoreSlot& sl = s->slots[i];
        if (sl.done) { (void)hipEventSynchronize(sl.done); (void)hipEventDestroy(sl.done); }
        if (sl.pin_arena) (void)hipHostFree(sl.pin_arena);
        if (sl.pin_scores) (void)hipHostFree(sl.pin_scores);
        if (sl.dev_arena) (void)hipFree(sl.dev_arena);
        if (sl.feats) (void)hipFree(sl.feats);
        if (sl.h) (void)hipFree(sl.h);
        if (sl.scores) (void)hipFree(sl.scores);
    }
    delete[] s->slots;
    delete s;
}

}  // namespace

extern "C" void* forge_rescore_new(
    const void* w1t, const void* b1, const void* w2t, const void* b2,
    int dim, int hidden, int classes, int max_rows, int64_t max_bytes, int n_slots)
{
    if (max_rows <= 0) max_rows = 1024;
    if (max_bytes <= 0) max_bytes = (int64_t)512 * max_rows;
    if (n_slots <= 0) n_slots = 4;
    // dim: featurize buckets with & (dim-1) and the v1 GEMM needs K%64;
    // hidden: N%128 for the v1 GEMM, K%512 for the gemv head
    if (w1t == nullptr || w2t == nullptr || dim < 64 || (dim & (dim - 1)) || hidden <= 0 ||
        (hidden % 128) || (hidden % (WAVE * 8)) || classes <= 0 || classes > 32 ||
        max_bytes > ((int64_t)1 << 30))
        return nullptr;

    RescoreSession* s = new (std::nothrow) RescoreSession();
    if (s == nullptr) return nullptr;
    s->w1t = w1t; s->b1 = b1; s->w2t = w2t; s->b2 = b2;
    s->dim = dim; s->hidden = hidden; s->classes = classes;
    s->max_rows = max_rows; s->rows_cap = round_up(max_rows, 128);
    s->n_slots = n_slots; s->max_bytes = max_bytes;
    s->bytes_off = ((int64_t)(max_rows + 1) * 4 + 15) & ~(int64_t)15;
    const char* env = getenv("FORGE_GEMM_SKINNY");
    s->skinny = !(env != nullptr && env[0] == '0' && env[1] == '\0');
    s->slots = new (std::nothrow) RescoreSlot[n_slots];
    if (s->slots == nullptr) { delete s; return nullptr; }

    const size_t arena = (size_t)(s->bytes_off + max_bytes);
    const size_t feats_b = (size_t)s->rows_cap * dim * 2;
    bool ok = true;
    for (int i = 0; ok && i < n_slots; ++i) {
        RescoreSlot& sl = s->slots[i];
        ok = hipHostMalloc((void**)&sl.pin_arena, arena, hipHostMallocDefault) == hipSuccess
          && hipHostMalloc((void**)&sl.pin_scores, (size_t)max_rows * classes * 4, hipHostMallocDefault) == hipSuccess
          && hipMalloc((void**)&sl.dev_arena, arena) == hipSuccess
          && hipMalloc((void**)&sl.feats, feats_b) == hipSuccess
          && hipMalloc((void**)&sl.h, (size_t)s->rows_cap * hidden * 2) == hipSuccess
          && hipMalloc((void**)&sl.scores, (size_t)s->rows_cap * classes * 4) == hipSuccess
          && hipMemset(sl.feats, 0, feats_b) == hipSuccess
          && hipEventCreateWithFlags(&sl.done, hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) { (void)hipGetLastError(); free_session(s); return nullptr; }
    return s;
}

extern "C" int forge_rescore_submit(void* ctx, const uint8_t* blob, const int64_t* offs, int n, void* stream)
{
    RescoreSession* s = (RescoreSession*)ctx;
    if (s == nullptr || blob == nullptr || offs == nullptr || n <= 0 || n > s->max_rows)
        return -FORGE_ERR_RESCORE_ARGS;
    const int64_t base = offs[0];
    if (base < 0) return -FORGE_ERR_RESCORE_ARGS;
    for (int i = 0; i < n; ++i)
        if (offs[i + 1] < offs[i]) return -FORGE_ERR_RESCORE_ARGS;
    const int64_t total = offs[n] - base;
    if (total > s->max_bytes) return -FORGE_ERR_RESCORE_ARGS;

    int slot = -1;
    for (int i = 0; i < s->n_slots && slot < 0; ++i) {
        RescoreSlot& sl = s->slots[i];
        // released while its work was still in flight: free once that is done
        if (sl.state == SLOT_DRAINING && hipEventQuery(sl.done) == hipSuccess) sl.state = SLOT_FREE;
        if (sl.state == SLOT_FREE) slot = i;
    }
    (void)hipGetLastError();  // hipErrorNotReady of a draining slot is no error
    if (slot < 0) return -FORGE_ERR_RESCORE_BUSY;
    RescoreSlot& sl = s->slots[slot];
    hipStream_t st = (hipStream_t)stream;

    int32_t* o32 = (int32_t*)sl.pin_arena;
    for (int i = 0; i <= n; ++i) o32[i] = (int32_t)(offs[i] - base);
    memcpy(sl.pin_arena + s->bytes_off, blob + base, (size_t)total);

    int rc = (int)hipMemcpyAsync(sl.dev_arena, sl.pin_arena, (size_t)(s->bytes_off + total),
                                 hipMemcpyHostToDevice, st);
    if (rc != 0) return -rc;
    const int32_t* d_offs = (const int32_t*)sl.dev_arena;
    rc = forge_featurize(sl.dev_arena + s->bytes_off, d_offs, d_offs + 1, n, s->dim, sl.feats, nullptr, stream);
    if (rc == 0) {
        if (s->skinny)
            rc = forge_gemm_bt_skinny(sl.feats, s->w1t, s->b1, sl.h, round_up(n, 64), s->hidden, s->dim,
                                      FORGE_ACT_GELU, 1, stream);
        else
            rc = forge_gemm_bt(sl.feats, s->w1t, s->b1, sl.h, round_up(n, 128), s->hidden, s->dim,
                               FORGE_ACT_GELU, 1, stream);
    }
    if (rc == 0)
        rc = forge_gemv_head(sl.h, s->w2t, s->b2, sl.scores, n, s->classes, s->hidden, FORGE_ACT_SIGMOID, stream);
    if (rc == 0)
        rc = (int)hipMemcpyAsync(sl.pin_scores, sl.scores, (size_t)n * s->classes * 4, hipMemcpyDeviceToHost, st);
    // the event is recorded even after a failed launch: the slot then drains
    // behind whatever did go out before it is handed out again
    int rc_ev = (int)hipEventRecord(sl.done, st);
    if (rc != 0 || rc_ev != 0) {
        sl.state = SLOT_DRAINING;
        return -(rc != 0 ? rc : rc_ev);
    }
    sl.state = SLOT_BUSY;
    return slot;
}

static RescoreSlot* rescore_slot(void* ctx, int slot) {
    RescoreSession* s = (RescoreSession*)ctx;
    if (s == nullptr || slot < 0 || slot >= s->n_slots) return nullptr;
    return &s->slots[slot];
}

extern "C" int forge_rescore_poll(void* ctx, int slot)
{
    RescoreSlot* sl = rescore_slot(ctx, slot);
    if (sl == nullptr || sl->state != SLOT_BUSY) return -FORGE_ERR_RESCORE_ARGS;
    hipError_t e = hipEventQuery(sl->done);
    if (e == hipSuccess) return 1;
    if (e == hipErrorNotReady) { (void)hipGetLastError(); return 0; }
    return -(int)e;
}

extern "C" int forge_rescore_wait(void* ctx, int slot)
{
    RescoreSlot* sl = rescore_slot(ctx, slot);
    if (sl == nullptr || sl->state != SLOT_BUSY) return -FORGE_ERR_RESCORE_ARGS;
    hipError_t e = hipEventSynchronize(sl->done);
    return e == hipSuccess ? 1 : -(int)e;
}

extern "C" const float* forge_rescore_scores(void* ctx, int slot)
{
    RescoreSlot* sl = rescore_slot(ctx, slot);
    return sl != nullptr ? sl->pin_scores : nullptr;
}

extern "C" void forge_rescore_release(void* ctx, int slot)
{
    RescoreSlot* sl = rescore_slot(ctx, slot);
    if (sl != nullptr && sl->state == SLOT_BUSY) sl->state = SLOT_DRAINING;
}

extern "C" void forge_rescore_free(void* ctx)
{
    free_session((RescoreSession*)ctx);
}
