// Python-free parts of the native HTTP edge (edge.cpp): the queued request,
// the hot/slow lane split + packing of a drained batch, and HTTP response
// framing. Header-only and free of <Python.h> so a stand-alone program can
// exercise them (edge_pack_driver.cpp runs them under ASan/UBSan).
//
// Lane split. A drained batch is split, in queue order, into
//   * the HOT lane — K_RPC rows whose user the C++ auth memo already
//     resolved, or that carry no Authorization header at all (such rows only
//     reach the queue when auth is not required). It is packed into flat
//     arrays: ids, one blob of all bodies back to back, int64 offsets
//     (h + 1 entries, the layout pybridge's concat_with_offsets produces) and
//     a per-row index into the batch's DISTINCT users. Users are interned
//     pointers, so distinctness is pointer identity.
//   * the SLOW lane — everything else (K_OTHER rows, K_RPC rows whose
//     Authorization header the memo has not resolved), kept per row.

#pragma once

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

namespace edgepack {

enum ReqKind : uint8_t { K_RPC = 0, K_OTHER = 1 };

struct Req {
    uint64_t id = 0;
    uint8_t kind = K_RPC;
    std::string body;
    const std::string* user = nullptr;  // interned; null = unresolved
    std::string authz;                  // raw header value when unresolved
    std::string method, target, headers_blob;  // K_OTHER only
};

inline bool is_hot(const Req& r) {
    return r.kind == K_RPC && (r.user != nullptr || r.authz.empty());
}

struct LanePlan {
    std::vector<uint32_t> hot;    // batch indices, queue order
    std::vector<uint32_t> slow;   // batch indices, queue order
    size_t blob_bytes = 0;        // sum of hot body sizes
    std::vector<int32_t> uidx;    // per hot row: index into users
    std::vector<const std::string*> users;  // distinct, first-seen order; may hold null
    std::vector<int64_t> ucount;  // hot rows per distinct user
};

// Split `batch` into lanes and dedupe the hot lane's users. No row is moved
// or copied; the plan only indexes into `batch`.
inline void plan_lanes(const std::vector<Req>& batch, LanePlan& p) {
    p.hot.clear();
    p.slow.clear();
    p.uidx.clear();
    p.users.clear();
    p.ucount.clear();
    p.blob_bytes = 0;
    p.hot.reserve(batch.size());
    p.uidx.reserve(batch.size());
    int32_t last = -1;
    for (size_t i = 0; i < batch.size(); ++i) {
        const Req& r = batch[i];
        if (!is_hot(r)) {
            p.slow.push_back((uint32_t)i);
            continue;
        }
        // nearly every row repeats the previous row's user; otherwise scan
        // the (short) distinct list
        int32_t u = -1;
        if (last >= 0 && p.users[(size_t)last] == r.user) {
            u = last;
        } else {
            for (size_t k = 0; k < p.users.size(); ++k)
                if (p.users[k] == r.user) { u = (int32_t)k; break; }
            if (u < 0) {
                u = (int32_t)p.users.size();
                p.users.push_back(r.user);
                p.ucount.push_back(0);
            }
            last = u;
        }
        p.ucount[(size_t)u]++;
        p.uidx.push_back(u);
        p.hot.push_back((uint32_t)i);
        p.blob_bytes += r.body.size();
    }
}

// Write the hot lane into caller-owned buffers: ids[h], blob[p.blob_bytes],
// offs[h + 1]. `blob` may be null when blob_bytes == 0.
inline void pack_hot(const std::vector<Req>& batch, const LanePlan& p,
                     uint64_t* ids, char* blob, int64_t* offs) {
    size_t at = 0;
    offs[0] = 0;
    for (size_t j = 0; j < p.hot.size(); ++j) {
        const Req& r = batch[p.hot[j]];
        ids[j] = r.id;
        if (!r.body.empty()) memcpy(blob + at, r.body.data(), r.body.size());
        at += r.body.size();
        offs[j + 1] = (int64_t)at;
    }
}

inline const char* reason_of(int code) {
    switch (code) {
        case 200: return "OK";
        case 202: return "Accepted";
        case 400: return "Bad Request";
        case 401: return "Unauthorized";
        case 403: return "Forbidden";
        case 404: return "Not Found";
        case 413: return "Payload Too Large";
        case 429: return "Too Many Requests";
        case 431: return "Request Header Fields Too Large";
        case 501: return "Not Implemented";
        default: return "Internal Server Error";
    }
}

inline void format_response(std::string& out, int code, const char* body, size_t n, bool keep_alive) {
    char head[160];
    int hn = snprintf(head, sizeof(head),
                      "HTTP/1.1 %d %s\r\nContent-Type: application/json\r\n"
                      "Content-Length: %zu\r\nConnection: %s\r\n\r\n",
                      code, reason_of(code), n, keep_alive ? "keep-alive" : "close");
    out.append(head, (size_t)hn);
    if (n) out.append(body, n);
}

}  // namespace edgepack
