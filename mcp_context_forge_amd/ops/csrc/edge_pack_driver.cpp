// Stand-alone driver for edge_pack.hpp (the Python-free parts of the native
// edge): runs the lane split, the hot-lane packing and the response framing
// over synthetic batches and checks them against a straightforward per-row
// reference. Built with -fsanitize=address,undefined by
// tests/test_edge_pack_sanitizer.py; exits non-zero on any mismatch.
//
//   edge_pack_driver [rows=600] [rounds=8]

#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "edge_pack.hpp"

using namespace edgepack;

static int fails = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            fails++;                                                       \
        }                                                                  \
    } while (0)

static uint32_t rng_state = 12345;
static uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

// mode 0: mixed; 1: all hot, one user; 2: all slow; 3: anonymous hot rows
static std::vector<Req> make_batch(size_t n, int mode, const std::vector<std::string>& interned) {
    std::vector<Req> b(n);
    for (size_t i = 0; i < n; ++i) {
        Req& r = b[i];
        r.id = ((uint64_t)rnd() << 32) | i;
        size_t len = (mode == 0 && rnd() % 7 == 0) ? 0 : rnd() % 300;
        r.body.assign(len, (char)('a' + i % 26));
        int pick = mode == 0 ? (int)(rnd() % 10) : mode == 1 ? 0 : mode == 2 ? 8 + (int)(i % 2) : 7;
        if (pick < 7) {            // resolved user (interleaved)
            r.user = &interned[mode == 1 ? 0 : rnd() % interned.size()];
        } else if (pick == 7) {    // no Authorization header at all
        } else if (pick == 8) {    // unresolved Authorization header
            r.authz = "Bearer tok" + std::to_string(i);
        } else {                   // control-plane request
            r.kind = K_OTHER;
            r.method = "GET";
            r.target = "/version";
            r.headers_blob = "GET /version HTTP/1.1\r\n\r\n";
            if (rnd() % 2) r.user = &interned[0];  // a user never makes K_OTHER hot
        }
    }
    return b;
}

static void check_batch(const std::vector<Req>& batch) {
    LanePlan p;
    plan_lanes(batch, p);
    CHECK(p.hot.size() + p.slow.size() == batch.size());
    CHECK(p.uidx.size() == p.hot.size());
    CHECK(p.users.size() == p.ucount.size());

    size_t h = p.hot.size();
    std::vector<uint64_t> ids(h);
    std::vector<char> blob(p.blob_bytes);
    std::vector<int64_t> offs(h + 1);
    pack_hot(batch, p, ids.data(), blob.data(), offs.data());

    // reference: walk the batch in queue order
    size_t hi = 0, si = 0;
    int64_t total = 0;
    std::vector<int64_t> count(p.users.size(), 0);
    for (size_t i = 0; i < batch.size(); ++i) {
        const Req& r = batch[i];
        bool hot = r.kind == K_RPC && (r.user != nullptr || r.authz.empty());
        if (!hot) {
            CHECK(si < p.slow.size() && p.slow[si] == i);
            si++;
            continue;
        }
        CHECK(hi < h && p.hot[hi] == i);
        if (hi >= h) break;
        CHECK(ids[hi] == r.id);
        CHECK(offs[hi] == total);
        CHECK((size_t)(offs[hi + 1] - offs[hi]) == r.body.size());
        CHECK(r.body.empty() || memcmp(blob.data() + offs[hi], r.body.data(), r.body.size()) == 0);
        int32_t u = p.uidx[hi];
        CHECK(u >= 0 && (size_t)u < p.users.size());
        if (u >= 0 && (size_t)u < p.users.size()) {
            CHECK(p.users[(size_t)u] == r.user);
            count[(size_t)u]++;
        }
        total += (int64_t)r.body.size();
        hi++;
    }
    CHECK(hi == h && si == p.slow.size());
    CHECK(offs[h] == total && (size_t)total == p.blob_bytes);
    int64_t sum = 0;
    for (size_t k = 0; k < p.users.size(); ++k) {
        CHECK(count[k] == p.ucount[k]);
        sum += p.ucount[k];
        for (size_t q = 0; q < k; ++q) CHECK(p.users[q] != p.users[k]);  // distinct
    }
    CHECK(sum == (int64_t)h);
}

static void check_format() {
    const int codes[] = {200, 202, 400, 401, 403, 404, 413, 429, 431, 501, 500, 599};
    std::string out;
    size_t at = 0;
    for (int code : codes) {
        for (int ka = 0; ka < 2; ++ka) {
            std::string body(code == 202 ? 0 : (size_t)(rnd() % 5000), 'x');
            format_response(out, code, body.data(), body.size(), ka != 0);
            std::string got = out.substr(at);
            at = out.size();
            char want[256];
            snprintf(want, sizeof(want),
                     "HTTP/1.1 %d %s\r\nContent-Type: application/json\r\n"
                     "Content-Length: %zu\r\nConnection: %s\r\n\r\n",
                     code, reason_of(code), body.size(), ka ? "keep-alive" : "close");
            CHECK(got == std::string(want) + body);
        }
    }
    // a null body pointer with zero length (None -> 202) must be fine
    std::string o2;
    format_response(o2, 202, nullptr, 0, true);
    CHECK(o2.find("202 Accepted") != std::string::npos && o2.find("Content-Length: 0\r\n") != std::string::npos);
}

int main(int argc, char** argv) {
    size_t rows = argc > 1 ? (size_t)atoi(argv[1]) : 600;
    int rounds = argc > 2 ? atoi(argv[2]) : 8;
    std::vector<std::string> interned = {"alice@example.com", "bob@example.com", "carol@example.com"};
    std::vector<std::string> many;
    for (int i = 0; i < 40; ++i) many.push_back("user" + std::to_string(i) + "@example.com");

    check_batch({});  // empty queue
    for (int mode = 0; mode < 4; ++mode) {
        check_batch(make_batch(1, mode, interned));
        for (int r = 0; r < rounds; ++r) {
            check_batch(make_batch(rows + (size_t)r, mode, interned));
            check_batch(make_batch(rows / 3 + 1, mode, many));
        }
    }
    check_format();
    if (fails) {
        fprintf(stderr, "edge pack driver: %d check(s) failed\n", fails);
        return 1;
    }
    printf("edge pack driver ok\n");
    return 0;
}
