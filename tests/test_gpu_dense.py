"""The GEMM, row and scan kernels against exact-integer and float64 oracles
(tests/kernel_oracles.py; the oracles and inputs themselves are checked on the
CPU by tests/test_kernel_oracles.py).

Integer cases have no tolerance: inputs in -4..4 keep every partial sum below
2^24, so every fp32 accumulation order is exact. Random cases assert a bound
derived from the number formats and, for the MFMA GEMMs and the activations,
ten times the error measured on an MI355X (docs/kernels.md, "Numerics of the
dense kernels"); each prints its measured figure before it asserts.
"""

import numpy as np
import pytest
import torch

import kernel_oracles as ko
from mcp_context_forge_amd.ops.featurize import featurize_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from mcp_context_forge_amd.ops import hip as _hip

    if not _hip.available():
        pytest.fail("libforge_hip must load on a GPU box (no silent fallback)")
    return _hip


def _act_code(hip, act):
    return {"none": hip.ACT_NONE, "gelu": hip.ACT_GELU, "sigmoid": hip.ACT_SIGMOID}[act]


def _gemm(hip, monkeypatch, kernel, a, bt, bias=None, act="none", out_bf16=False):
    """Run one of the three GEMMs on CPU operands; → the result on the CPU."""
    args = (a.cuda(), bt.cuda(), bias.cuda() if bias is not None else None)
    kw = dict(act=_act_code(hip, act), out_bf16=out_bf16)
    if kernel == "skinny":
        return hip.gemm_bt_skinny(*args, **kw).cpu()
    if kernel == "v1":
        monkeypatch.setenv("FORGE_GEMM_V1", "1")
    else:
        monkeypatch.delenv("FORGE_GEMM_V1", raising=False)
        assert a.shape[0] % 256 == 0 and bt.shape[0] % 256 == 0 and a.shape[1] % 32 == 0   # the dispatcher picks v2
    return hip.gemm_bt(*args, **kw).cpu()


def _bits16(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------
# GEMM: integer cases, no tolerance
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kernel,m,n,k", ko.GEMM_CASES)
def test_gemm_integer_exact(hip, monkeypatch, kernel, m, n, k):
    a, bt, bias, ref, ref_b = ko.int_gemm_case(m, n, k)
    for b, r in ((None, ref), (bias, ref_b)):
        want = r.float()
        got = _gemm(hip, monkeypatch, kernel, a, bt, b)
        assert got.dtype == torch.float32
        assert torch.equal(got, want), (int((got != want).sum()), (got - want).abs().max().item())
        # odd integers in [256, 512) and their like are exact ties: this pins round-to-nearest-even
        got16 = _gemm(hip, monkeypatch, kernel, a, bt, b, out_bf16=True)
        assert got16.dtype == torch.bfloat16
        assert torch.equal(_bits16(got16), _bits16(want.bfloat16())), int((got16 != want.bfloat16()).sum())


# ---------------------------------------------------------------------------
# GEMM: the bf16 store is the rounded fp32 store
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", sorted(ko.EPILOGUE_SHAPES))
@pytest.mark.parametrize("act", ko.ACTS)
@pytest.mark.parametrize("has_bias", [False, True], ids=["nobias", "bias"])
def test_gemm_bf16_store_equals_rounded_f32_store(hip, monkeypatch, kernel, act, has_bias):
    a, bt, bias, _ = ko.epilogue_case(kernel)
    b = bias if has_bias else None
    f32 = _gemm(hip, monkeypatch, kernel, a, bt, b, act)
    b16 = _gemm(hip, monkeypatch, kernel, a, bt, b, act, out_bf16=True)
    assert torch.equal(_bits16(b16), _bits16(f32.bfloat16()))


# ---------------------------------------------------------------------------
# GEMM: rounding error on random inputs, against float64
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kernel,m,n,k", ko.GEMM_CASES)
def test_gemm_rounding_error(hip, monkeypatch, kernel, m, n, k):
    a, bt, ref, ad = ko.random_gemm_case(kernel, m, n, k)
    got = _gemm(hip, monkeypatch, kernel, a, bt).double()
    err = (got - ref).abs()
    rel = (err / ad).max().item()
    print(f"MEASURED gemm {kernel} {m}x{n}x{k}: max|got-ref|/abs_dot = {rel:.3e} "
          f"(hard {k * ko.GEMM_HARD_EPS:.3e}, working {ko.gemm_working_bound(kernel):.3e})")
    assert bool((err <= k * ko.GEMM_HARD_EPS * ad).all())            # derived
    assert rel <= ko.gemm_working_bound(kernel)                        # measured x 10
    # ... and that working bound tells an fp32 epilogue from a bf16 round trip
    big = ref.abs() >= 1.0
    assert bool((ko.gemm_working_bound(kernel) * ad[big] < ko.BF16_HALF_ULP * ref.abs()[big]).all())


# ---------------------------------------------------------------------------
# GEMM: bias and activation, isolated from the matmul
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", sorted(ko.EPILOGUE_SHAPES))
@pytest.mark.parametrize("act", ko.ACTS)
@pytest.mark.parametrize("has_bias", [False, True], ids=["nobias", "bias"])
def test_gemm_epilogue_against_float64(hip, monkeypatch, kernel, act, has_bias):
    a, bt, bias, refs = ko.epilogue_case(kernel)
    k = a.shape[1]
    ad = ko.abs_dot(a, bt)
    ref = refs[(act, has_bias)]
    # no other (act, bias) wiring can pass: each is >= 4 tolerances away
    loose = ko.epilogue_tol(k * ko.GEMM_HARD_EPS, ad, refs[("none", has_bias)], "gemm", act)
    assert ko.wiring_separation(refs, (act, has_bias), loose) >= 1.0
    b = bias if has_bias else None
    z = _gemm(hip, monkeypatch, kernel, a, bt, b).double()
    # the pre-activation: K adds of the accumulator and one of the bias
    zref = refs[("none", has_bias)]
    assert bool(((z - zref).abs() <= k * ko.GEMM_HARD_EPS * ad + 2.0 ** -23 * zref.abs()).all())
    got = _gemm(hip, monkeypatch, kernel, a, bt, b, act).double()
    if act == "none":
        return
    # the activation alone: float64 of the kernel's own pre-activation
    want = ko.act_ref(z, act)
    err = ((got - want).abs() / want.abs().clamp(min=1.0)).max().item()
    print(f"MEASURED act gemm {kernel} {act} bias={has_bias}: {err:.3e} (bound {ko.act_bound('gemm', act):.3e})")
    assert err <= ko.act_bound("gemm", act)
    # and the whole epilogue lands on this reference, not on another wiring's
    assert bool(((got - ref).abs() <= loose(ref)).all())


# ---------------------------------------------------------------------------
# GEMM: a NaN through the bf16 store
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", sorted(ko.EPILOGUE_SHAPES))
def test_gemm_nan_survives_the_bf16_store(hip, monkeypatch, kernel):
    a, bt, bias, _ = ko.epilogue_case(kernel)
    a = a.clone()
    a[3, 17] = float("nan")
    for b in (None, bias):
        f32 = _gemm(hip, monkeypatch, kernel, a, bt, b)
        b16 = _gemm(hip, monkeypatch, kernel, a, bt, b, out_bf16=True)
        assert bool(f32[3].isnan().all()) and int(f32.isnan().sum()) == f32.shape[1]
        assert torch.equal(b16.isnan(), f32.isnan())
    # the NaN whose mantissa is all ones: the rounding add used to wrap it to -0.0
    a, bt, bias, _ = ko.epilogue_case(kernel)
    bias = bias.clone()
    bias.view(torch.int32)[5] = 0x7FFFFFFF
    bias.view(torch.int32)[6] = -1
    f32 = _gemm(hip, monkeypatch, kernel, a, bt, bias)
    b16 = _gemm(hip, monkeypatch, kernel, a, bt, bias, out_bf16=True)
    assert bool(f32[:, 5:7].isnan().all()) and int(f32.isnan().sum()) == 2 * f32.shape[0]
    assert torch.equal(b16.isnan(), f32.isnan())


# ---------------------------------------------------------------------------
# gemv_head
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("m,c,k", ko.GEMV_SHAPES)
def test_gemv_head_integer_exact(hip, m, c, k):
    a, wt, bias, ref, ref_b = ko.int_gemm_case(m, c, k)
    for b, r in ((None, ref), (bias, ref_b)):
        got = hip.gemv_head(a.cuda(), wt.cuda(), b.cuda() if b is not None else None, act=hip.ACT_NONE).cpu()
        assert torch.equal(got, r.float())


@pytest.mark.parametrize("m,c,k", ko.GEMV_SHAPES)
@pytest.mark.parametrize("act", ko.ACTS)
@pytest.mark.parametrize("has_bias", [False, True], ids=["nobias", "bias"])
def test_gemv_head_against_float64(hip, m, c, k, act, has_bias):
    a, wt, bias, refs = ko.gemv_case(m, c, k)
    ad = ko.abs_dot(a, wt)
    ref = refs[(act, has_bias)]
    loose = ko.epilogue_tol(k * ko.DOT_EPS, ad, refs[("none", has_bias)], "gemv", act)
    assert ko.wiring_separation(refs, (act, has_bias), loose) >= 1.0
    b = bias.cuda() if has_bias else None
    z = hip.gemv_head(a.cuda(), wt.cuda(), b, act=hip.ACT_NONE).cpu().double()
    zref = refs[("none", has_bias)]
    zerr = (z - zref).abs()
    print(f"MEASURED gemv_head {m}x{c}x{k} bias={has_bias}: max|got-ref|/abs_dot = {(zerr / ad).max().item():.3e} "
          f"(derived {k * ko.DOT_EPS:.3e})")
    # derived: plain fp32 adds, round to nearest; one more add for the bias
    assert bool((zerr <= k * ko.DOT_EPS * ad + (2.0 ** -23 * zref.abs() if has_bias else 0.0)).all())
    if act == "none":
        return
    got = hip.gemv_head(a.cuda(), wt.cuda(), b, act=_act_code(hip, act)).cpu().double()
    want = ko.act_ref(z, act)
    err = ((got - want).abs() / want.abs().clamp(min=1.0)).max().item()
    print(f"MEASURED act gemv {m}x{c}x{k} {act} bias={has_bias}: {err:.3e} (bound {ko.act_bound('gemv', act):.3e})")
    assert err <= ko.act_bound("gemv", act)
    assert bool(((got - ref).abs() <= loose(ref)).all())


# ---------------------------------------------------------------------------
# verify_dot
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("d", ko.VERIFY_DOT_D)
@pytest.mark.parametrize("m", ko.VERIFY_DOT_M)
def test_verify_dot_integer_exact(hip, m, d):
    feats, keys, idx, ref = ko.int_verify_dot_case(m, d)
    got = hip.verify_dot(feats.cuda(), keys.cuda(), idx.cuda()).cpu().numpy()
    np.testing.assert_array_equal(got, ref)     # idx = -1 rows are float32(-1e30) exactly


@pytest.mark.parametrize("d", ko.VERIFY_DOT_D)
def test_verify_dot_rounding_error(hip, d):
    m, cap = 5, 6
    feats, keys = ko.random_operands(m, cap, d, seed=61 + d, scale=0.3)
    idx = torch.tensor([4, -1, 0, 5, 2], dtype=torch.int32)
    got = hip.verify_dot(feats.cuda(), keys.cuda(), idx.cuda()).cpu().double()
    full, ad = ko.gemm_ref(feats, keys), ko.abs_dot(feats, keys)
    worst = 0.0
    for i, s in enumerate(idx.tolist()):
        if s < 0:
            assert got[i].item() == float(ko.SENTINEL)
            continue
        err = abs(got[i].item() - full[i, s].item())
        worst = max(worst, err / ad[i, s].item())
        assert err <= d * ko.DOT_EPS * ad[i, s].item()            # derived
    print(f"MEASURED verify_dot D={d}: max|got-ref|/abs_dot = {worst:.3e} (derived {d * ko.DOT_EPS:.3e})")


# ---------------------------------------------------------------------------
# rows_argmax_merge. NaN scores are out of scope: the kernel's compares are
# all false on a NaN and the semantic cache never produces one.
# ---------------------------------------------------------------------------

def _merge_gpu(hip, scores, valid_buf, idx_base, best_val, best_idx):
    bv, bi = torch.from_numpy(best_val.copy()).cuda(), torch.from_numpy(best_idx.copy()).cuda()
    nc = scores.shape[1]
    valid = None
    if valid_buf is not None:
        # a slice at an offset that is no multiple of 4, as semcache passes slices
        valid = torch.from_numpy(valid_buf).cuda()[ko.VALID_OFFSET:ko.VALID_OFFSET + nc]
        assert valid.data_ptr() % 4 != 0
    hip.rows_argmax_merge(torch.from_numpy(scores).cuda(), bv, bi, idx_base=idx_base, valid=valid)
    torch.cuda.synchronize()
    return bv.cpu().numpy(), bi.cpu().numpy()


@pytest.mark.parametrize("nc", ko.ARGMAX_NC)
@pytest.mark.parametrize("m", ko.ARGMAX_M)
def test_rows_argmax_merge_matches_reference(hip, m, nc):
    scores = ko.argmax_scores(m, nc, seed=100 * m + nc)
    rng = np.random.default_rng(m + nc)
    initial = (np.full(m, ko.SENTINEL, dtype=np.float32), np.full(m, -1, dtype=np.int32))
    # a carried best from an earlier chunk: below, equal to and above this chunk's values
    carried = (np.concatenate([ko.ARGMAX_VALUES, [np.float32(100.0)]])[rng.integers(0, 5, size=m)].astype(np.float32),
               rng.integers(0, 900, size=m).astype(np.int32))
    for kind in ("none", "random", "ones", "zeros"):
        buf = ko.argmax_valid(kind, nc, seed=nc)
        valid = None if buf is None else buf[ko.VALID_OFFSET:ko.VALID_OFFSET + nc]
        for bv0, bi0 in (initial, carried):
            want_v, want_i = ko.argmax_merge_ref(scores, valid, 1000, bv0, bi0)
            got_v, got_i = _merge_gpu(hip, scores, buf, 1000, bv0, bi0)
            np.testing.assert_array_equal(got_i, want_i, err_msg=f"{kind} idx")
            np.testing.assert_array_equal(got_v.view(np.int32), want_v.view(np.int32), err_msg=f"{kind} val")
            if kind == "zeros":   # nothing valid: the carried pair stays, bit for bit
                np.testing.assert_array_equal(got_i, bi0)
                np.testing.assert_array_equal(got_v.view(np.int32), bv0.view(np.int32))


@pytest.mark.parametrize("nc", [64, 257, 1024])
def test_rows_argmax_merge_three_chunk_fold(hip, nc):
    """The chunked sweep of gpu/semcache.py: ascending idx_base, the global
    maximum tied between chunk 0 and chunk 2 — chunk 0's index wins."""
    m = 5
    chunks = [ko.argmax_scores(m, nc, seed=7 * nc + c) for c in range(3)]
    top = np.float32(9.5)
    for r in range(m):
        chunks[0][r, (11 * r + 3) % nc] = top
        chunks[2][r, (5 * r + 1) % nc] = top
    bufs = [ko.argmax_valid("ones", nc, seed=1), ko.argmax_valid("random", nc, seed=2), None]
    want = gv = (np.full(m, ko.SENTINEL, dtype=np.float32), np.full(m, -1, dtype=np.int32))
    for c in range(3):
        valid = None if bufs[c] is None else bufs[c][ko.VALID_OFFSET:ko.VALID_OFFSET + nc]
        want = ko.argmax_merge_ref(chunks[c], valid, c * nc, *want)
        gv = _merge_gpu(hip, chunks[c], bufs[c], c * nc, *gv)
        np.testing.assert_array_equal(gv[1], want[1])
        np.testing.assert_array_equal(gv[0], want[0])
    np.testing.assert_array_equal(gv[1], [(11 * r + 3) % nc for r in range(m)])
    np.testing.assert_array_equal(gv[0], np.full(m, top))


def test_rows_argmax_merge_keeps_an_unbeaten_best(hip):
    m = 6
    bv0 = np.full(m, 50.0, dtype=np.float32)
    bi0 = np.arange(m, dtype=np.int32) + 7
    for nc in (63, 64):
        for c in range(3):
            got_v, got_i = _merge_gpu(hip, ko.argmax_scores(m, nc, seed=c), None, 100 * c, bv0, bi0)
            np.testing.assert_array_equal(got_v, bv0)
            np.testing.assert_array_equal(got_i, bi0)


# ---------------------------------------------------------------------------
# rows_gather_scatter_bf16. No duplicate slots: that outcome is a race and
# unspecified.
# ---------------------------------------------------------------------------

def _gather_case(d, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(-32768, 32768, (9, d), generator=g, dtype=torch.int32).to(torch.int16)
    src[0, 0], src[3, d - 1], src[4, d // 2], src[8, 1] = 0x7FC1, -1, 0x7F81, -64   # NaN encodings
    cap = 12
    dst = ((torch.arange(cap * d, dtype=torch.int32) * 37) % 30011 + 1).to(torch.int16).view(cap, d)
    return src, dst


@pytest.mark.parametrize("d", [8, 64, 2048, 2056, 4096])
@pytest.mark.parametrize("with_valid", [True, False], ids=["valid", "novalid"])
def test_rows_gather_scatter(hip, d, with_valid):
    src, dst0 = _gather_case(d, seed=d)
    rows = [3, -1, 8, 0, 5, 4]
    slots = [10, 4, 0, 11, -1, 7]
    live = [(r, s) for r, s in zip(rows, slots) if r >= 0 and s >= 0]
    dst = dst0.clone().cuda()
    valid = torch.zeros(dst0.shape[0], dtype=torch.uint8).cuda() if with_valid else None
    hip.rows_gather_scatter_bf16(src.cuda().view(torch.bfloat16), torch.tensor(rows, dtype=torch.int32).cuda(),
                                 torch.tensor(slots, dtype=torch.int32).cuda(), dst.view(torch.bfloat16), valid)
    torch.cuda.synchronize()
    want = dst0.clone()
    for r, s in live:
        want[s] = src[r]
    assert torch.equal(dst.cpu(), want)      # named rows copied bit for bit, every other row untouched
    if with_valid:
        want_valid = torch.zeros(dst0.shape[0], dtype=torch.uint8)
        want_valid[[s for _, s in live]] = 1
        assert torch.equal(valid.cpu(), want_valid)   # a skipped pair sets no validity, not even at slot 4


@pytest.mark.parametrize("d", [8, 2056])
def test_rows_gather_scatter_one_row(hip, d):
    src, dst0 = _gather_case(d, seed=d + 1)
    dst = dst0.clone().cuda()
    valid = torch.zeros(dst0.shape[0], dtype=torch.uint8).cuda()
    hip.rows_gather_scatter_bf16(src.cuda().view(torch.bfloat16), torch.tensor([8], dtype=torch.int32).cuda(),
                                 torch.tensor([6], dtype=torch.int32).cuda(), dst.view(torch.bfloat16), valid)
    want = dst0.clone()
    want[6] = src[8]
    assert torch.equal(dst.cpu(), want)
    assert valid.cpu().tolist() == [0] * 6 + [1] + [0] * 5


def test_rows_gather_scatter_refuses_unaligned_rows(hip):
    d = 12
    src = torch.ones(4, d, dtype=torch.bfloat16).cuda()
    dst = torch.full((4, d), 7.0, dtype=torch.bfloat16).cuda()
    valid = torch.zeros(4, dtype=torch.uint8).cuda()
    with pytest.raises(hip.ForgeHipError, match="9004"):     # FORGE_ERR_ROW_ALIGN
        hip.rows_gather_scatter_bf16(src, torch.tensor([1], dtype=torch.int32).cuda(),
                                     torch.tensor([2], dtype=torch.int32).cuda(), dst, valid)
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all()) and int(valid.sum()) == 0


# ---------------------------------------------------------------------------
# featurize
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dim", ko.FEATURIZE_DIMS)
def test_featurize_chunk_edges(hip, dim):
    blob, beg, end = ko.featurize_case()
    counts = ko.featurize_counts(dim)
    data = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    beg_t, end_t = torch.from_numpy(beg).cuda(), torch.from_numpy(end).cuda()
    out_bf16, out_f32 = hip.featurize(data, beg_t, end_t, dim, want_f32=True)
    torch.cuda.synchronize()
    got = out_f32.cpu().numpy()
    ref = featurize_batch([blob[b:e] for b, e in zip(beg, end)], dim)
    np.testing.assert_allclose(got, ref, atol=ko.FEATURIZE_ATOL)
    # the integer counts, exactly
    norms = np.sqrt((counts.astype(np.float64) ** 2).sum(axis=1))
    assert ko.FEATURIZE_ATOL * norms.max() < 0.5
    np.testing.assert_array_equal(np.rint(got.astype(np.float64) * norms[:, None]).astype(np.int64), counts)
    assert not got[norms == 0].any()
    # the bf16 store is the rounded fp32 store
    assert torch.equal(_bits16(out_bf16.cpu()), _bits16(out_f32.cpu().bfloat16()))
    # out= and pad_to= equal the plain path bit for bit; pad rows are zero
    pre = torch.full((len(beg), dim), 7.0, dtype=torch.bfloat16).cuda()
    same, none = hip.featurize(data, beg_t, end_t, dim, out=pre)
    assert same is pre and none is None
    assert torch.equal(_bits16(pre.cpu()), _bits16(out_bf16.cpu()))
    pad16, pad32 = hip.featurize(data, beg_t, end_t, dim, want_f32=True, pad_to=128)
    assert pad16.shape == (128, dim) and pad32.shape == (128, dim) and len(beg) < 128
    assert torch.equal(_bits16(pad16[:len(beg)].cpu()), _bits16(out_bf16.cpu()))
    assert torch.equal(pad32[:len(beg)].cpu().view(torch.int32), out_f32.cpu().view(torch.int32))
    assert not _bits16(pad16[len(beg):].cpu()).any() and not pad32[len(beg):].cpu().view(torch.int32).any()


# ---------------------------------------------------------------------------
# scan / scan_multi
# ---------------------------------------------------------------------------

def test_scan_first_end_on_the_corpus(hip):
    from mcp_context_forge_amd.gpu.batch import pack_texts
    from mcp_context_forge_amd.ops import dfa

    tables = dfa.compile_patterns(ko.SCAN_PATTERNS, case_insensitive=False)
    rows = ko.scan_corpus()
    data, beg, end = pack_texts(rows, "cuda")
    mask, first = hip.scan(data, beg, end, hip.DeviceScanTables(tables), first_end=True)
    torch.cuda.synchronize()
    mask, first = mask.cpu().numpy().view(np.uint32), first.cpu().numpy()
    for i, row in enumerate(rows):
        assert int(first[i]) == ko.first_end_ref(tables, row), (i, row)
        assert int(mask[i]) == dfa.match_mask_reference(tables, row), (i, row)
    assert (first > 0).sum() >= 4 and (first == -1).sum() >= 4


@pytest.fixture(scope="module")
def scan32():
    """Two 32-literal banks (tables in LDS / read through L2), 257 rows with
    gaps between the spans, and the reference of every row."""
    from mcp_context_forge_amd.ops import dfa
    from mcp_context_forge_amd.ops import hip

    out = {}
    for name, length in (("lds", 6), ("l2", 40)):
        words = ko.literal_words_32(length, seed=21)
        tables = dfa.compile_literals(words, True)
        assert (hip.scan_table_bytes(tables.n_states, tables.n_classes) <= hip.SCAN_LDS_LIMIT) == (name == "lds")
        rows = ko.scan32_rows(words, 257, seed=4)
        # the filler between the spans holds hits of other patterns: reading outside a span shows
        blob, beg, end = ko.gapped_spans(rows, (words[5] + " \xe9 " + words[9] + " ").encode("latin-1"), first_begin=13)
        masks = np.array([dfa.match_mask_reference(tables, r) for r in rows], dtype=np.uint32)
        firsts = np.array([ko.first_end_ref(tables, r) for r in rows], dtype=np.int32)
        out[name] = (tables, blob, beg, end, masks, firsts)
    return out


@pytest.mark.parametrize("bank", ["lds", "l2"])
@pytest.mark.parametrize("batch", [1, 255, 256, 257])
def test_scan_32_literals_gapped_spans(hip, scan32, bank, batch):
    tables, blob, beg, end, masks, firsts = scan32[bank]
    data = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    # batch 1 is the 20 KB row: bits 0 and 31, the first match in its last bytes
    sel = slice(7, 8) if batch == 1 else slice(0, batch)
    beg_t, end_t = torch.from_numpy(beg[sel].copy()).cuda(), torch.from_numpy(end[sel].copy()).cuda()
    mask, first = hip.scan(data, beg_t, end_t, hip.DeviceScanTables(tables), first_end=True)
    torch.cuda.synchronize()
    got = mask.cpu().numpy().view(np.uint32)       # bit 31 is the sign bit of the int32 tensor
    np.testing.assert_array_equal(got, masks[sel])
    np.testing.assert_array_equal(first.cpu().numpy(), firsts[sel])
    assert int(masks[7]) == 0x80000001 and end[7] - beg[7] == 20000 and beg[0] == 13


@pytest.mark.parametrize("batch", [1, 255, 256, 257])
def test_scan_multi_overwrites_a_garbage_out(hip, scan32, batch):
    t_lds, blob, beg, end, m_lds, _ = scan32["lds"]
    t_l2 = scan32["l2"][0]
    # both banks over the LDS bank's blob: the L2 bank's words do not occur in it
    from mcp_context_forge_amd.ops import dfa

    sel = slice(7, 8) if batch == 1 else slice(0, batch)
    data = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    beg_t, end_t = torch.from_numpy(beg[sel].copy()).cuda(), torch.from_numpy(end[sel].copy()).cuda()
    bs = hip.ScanBankSet([("lds", hip.DeviceScanTables(t_lds)), ("l2", hip.DeviceScanTables(t_l2))])
    out = torch.full((2, batch), 0x5A5A5A5A, dtype=torch.int32).cuda()
    got = hip.scan_multi(data, beg_t, end_t, bs, out=out)
    torch.cuda.synchronize()
    assert got is out
    got = out.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got[0], m_lds[sel])
    want_l2 = np.array([dfa.match_mask_reference(t_l2, blob[b:e]) for b, e in zip(beg[sel], end[sel])], dtype=np.uint32)
    np.testing.assert_array_equal(got[1], want_l2)


# ---------------------------------------------------------------------------
# Empty batches: nothing is launched, nothing is written, no error is left behind
# ---------------------------------------------------------------------------

def _empty_spans():
    data = torch.zeros(16, dtype=torch.uint8).cuda()
    none = torch.zeros(0, dtype=torch.int32).cuda()
    return data, none, none.clone()


def _device_still_fine():
    torch.cuda.synchronize()
    assert int(torch.arange(4).cuda().sum()) == 6


def test_empty_scan(hip):
    from mcp_context_forge_amd.ops import dfa

    data, beg, end = _empty_spans()
    mask, first = hip.scan(data, beg, end, hip.DeviceScanTables(dfa.compile_literals(["secret"])), first_end=True)
    assert mask.shape == (0,) and first.shape == (0,)
    _device_still_fine()


def test_empty_featurize(hip):
    data, beg, end = _empty_spans()
    out16, out32 = hip.featurize(data, beg, end, 512, want_f32=True)
    assert out16.shape == (0, 512) and out32.shape == (0, 512)
    pre = torch.full((2, 512), 7.0, dtype=torch.bfloat16).cuda()
    hip.featurize(data, beg, end, 512, out=pre)
    _device_still_fine()
    assert bool((pre == 7.0).all())


def test_empty_json_guard(hip):
    data, beg, end = _empty_spans()
    status, depth = hip.json_guard(data, beg, end)
    assert status.shape == (0,) and depth.shape == (0,)
    _device_still_fine()


def test_empty_gemv_head(hip):
    a = torch.zeros(0, 512, dtype=torch.bfloat16).cuda()
    wt = torch.ones(8, 512, dtype=torch.bfloat16).cuda()
    assert hip.gemv_head(a, wt).shape == (0, 8)
    pre = torch.full((2, 8), 7.0).cuda()
    hip.gemv_head(a, wt, out=pre)
    _device_still_fine()
    assert bool((pre == 7.0).all())


def test_empty_rows_argmax_merge(hip):
    bv, bi = torch.full((3,), 2.5).cuda(), torch.tensor([4, 5, 6], dtype=torch.int32).cuda()
    hip.rows_argmax_merge(torch.zeros(0, 8).cuda(), bv, bi, idx_base=10, valid=torch.ones(8, dtype=torch.uint8).cuda())
    _device_still_fine()
    assert bv.cpu().tolist() == [2.5] * 3 and bi.cpu().tolist() == [4, 5, 6]


def test_empty_verify_dot(hip):
    out = hip.verify_dot(torch.zeros(0, 64, dtype=torch.bfloat16).cuda(), torch.ones(4, 64, dtype=torch.bfloat16).cuda(),
                         torch.zeros(0, dtype=torch.int32).cuda())
    assert out.shape == (0,)
    _device_still_fine()


def test_empty_rows_gather_scatter(hip):
    src = torch.ones(4, 64, dtype=torch.bfloat16).cuda()
    dst = torch.full((4, 64), 7.0, dtype=torch.bfloat16).cuda()
    valid = torch.zeros(4, dtype=torch.uint8).cuda()
    none = torch.zeros(0, dtype=torch.int32).cuda()
    hip.rows_gather_scatter_bf16(src, none, none.clone(), dst, valid)
    _device_still_fine()
    assert bool((dst == 7.0).all()) and int(valid.sum()) == 0
