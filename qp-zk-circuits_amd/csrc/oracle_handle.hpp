// oracle_handle.hpp — the stage-level ABI's committed polynomial batch (include/qpgpu.h: qpgpu_oracle), shared by the entries
// that create it (oracle_api.cpp, oracle_sharded.cpp) and the ones that read its resident data in place (stage_api.cpp, fri_api.cpp). The
// qpgpu_challenger <-> Challenger conversion of the entries that take a transcript: challenger.hpp.
#pragma once
#include <memory>
#include "oracle_shard_map.hpp"
#include "prover_host.hpp"

// One shard of a coset-sharded oracle: a contiguous range of the leaves, resident on a context of its own.
struct OracleShard {
    qpgpu_ctx *ctx = nullptr;
    gl::u64 *block = nullptr;     // one allocation: [coeffs copy, shards 1..] | lde | digests | salt | salt key
    size_t block_words = 0;
    gl::u64 *coeffs = nullptr;    // shard 0 reads the home context's
    gl::u64 *lde = nullptr, *digests = nullptr, *salt = nullptr;   // [ncols][N/G], the subtree's levels, [4][N/G]
    uint32_t *d_key = nullptr;
};
struct OracleShards {
    qpgpu_ctx *home = nullptr;
    shard_map::Map map;
    bool blinded = false;
    std::vector<OracleShard> s;
    std::vector<gl::u64> merge;   // the home context's merge levels over the shards' roots (map.merge_digests() digests), host copy
};

struct qpgpu_oracle {
    qpgpu_ctx *ctx = nullptr;     // a sharded oracle's home context
    PolyOracle o;                 // sharded: coeffs on the home context, lde / digests / salt NULL, o.sh set
    gl::u64 *block = nullptr;     // one allocation: coeffs | lde | digests | salt | eval scratch | salt keys, each [o.nb][...]
    size_t block_words = 0;       // (sharded: coeffs | merge levels | eval scratch)
    gl::e2 *d_point = nullptr, *d_eval = nullptr;   // [nb] opening points, [nb][ncols] evaluations
    uint32_t *d_key = nullptr;                      // [nb][8]
    std::unique_ptr<OracleShards> sh;               // qpgpu_oracle_commit_sharded
};

// a failure on a shard's context is reported where the caller looks: on the home context
inline int shard_fail(qpgpu_ctx *home, uint32_t g, qpgpu_ctx *ctx, int rc) {
    if (ctx != home) home->err = "shard " + std::to_string(g) + ": " + ctx->err;
    return rc;
}
#define QP_SHARD(home, g, sctx, expr) do { int _rc = (expr); if (_rc) return shard_fail(home, g, sctx, _rc); } while (0)
#define QP_SHARD_HIP(home, g, sctx, call) do { hipError_t _e = (call); if (_e != hipSuccess) return shard_fail(home, g, sctx, (sctx)->hip_fail(_e, #call)); } while (0)

// the entries of oracle_api.cpp on a sharded oracle (oracle_sharded.cpp)
void oracle_sharded_free(qpgpu_oracle *h);
int oracle_sharded_read_lde(qpgpu_oracle *h, uint32_t first, uint32_t count, uint64_t *out);
// "<entry>: sharded oracles are not taken here yet ..." on the oracle's home context
int refuse_sharded(const qpgpu_oracle *h, const char *entry);
