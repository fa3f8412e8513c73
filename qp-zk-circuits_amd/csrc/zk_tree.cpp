// zk_tree.cpp — C ABI of the chain's 4-ary ZK Merkle tree on the device (include/qpgpu_leaf.h): a handle that keeps every level of a
// block's tree in HBM, its root, its levels and the Merkle paths of many leaves per call. The rules are common/src/zk_merkle.rs as
// leaf_witness.cpp restates them on the host; the geometry and the argument checks are zk_tree.hpp's, the kernels zk_tree_kernels.hip's.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>
#include "../../include/qpgpu_leaf.h"
#include "ctx.hpp"
#include "zk_tree.hpp"

static_assert(sizeof(qpgpu_zk_leaf) == zk_tree::LEAF_RECORD_BYTES, "qpgpu_zk_leaf is read by the kernel as six 64-bit words");
static_assert(QPGPU_ZK_TREE_MAX_LEAVES == zk_tree::MAX_LEAVES && QPGPU_LEAF_MAX_DEPTH == zk_tree::MAX_DEPTH &&
              QPGPU_ZK_TREE_FROM_TRANSFERS == zk_tree::FLAG_FROM_TRANSFERS, "qpgpu_leaf.h and zk_tree.hpp disagree");

static_assert(sizeof(qpgpu_zk_snapshot) == sizeof(zk_tree::Snapshot) && sizeof(qpgpu_zk_snapshot) == 16 + zk_tree::SNAPSHOT_NODES_BYTES &&
              offsetof(qpgpu_zk_snapshot, last) == offsetof(zk_tree::Snapshot, last), "qpgpu_zk_snapshot is copied into zk_tree::Snapshot whole");

struct qpgpu_zk_tree {
    qpgpu_ctx *ctx = nullptr;
    zk_tree::Plan plan;              // offsets laid out for `capacity`, sizes of the live count
    uint64_t capacity = 0;
    bool reserved = false;           // from qpgpu_zk_tree_build_reserved: appends are allowed
    uint8_t *d_nodes = nullptr;      // plan.total() nodes of 32 bytes, then Aux
    uint8_t *d_aux() const { return d_nodes + (size_t)plan.total() * zk_tree::NODE_BYTES; }
};

namespace {

// behind the nodes: the word that names a refused leaf and the snapshot nodes an append or a snapshot call gathers, read back in one copy
struct Aux {
    uint32_t bad_leaf, pad[7];       // (the nodes stay 32-byte aligned)
    uint8_t snap[zk_tree::SNAPSHOT_NODES_BYTES];
};

// a device allocation that lives for one call
struct Scratch {
    void *p = nullptr;
    ~Scratch() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
    template <class T> T *as() const { return (T *)p; }
};

int refuse(qpgpu_ctx *ctx, char *err, int code, const char *what, const char *why) {
    char msg[QPGPU_LEAF_ERR_CAP];
    std::snprintf(msg, sizeof msg, "%s: %s", what, why);
    if (err) std::snprintf(err, QPGPU_LEAF_ERR_CAP, "%s", msg);
    return ctx->fail(code, msg);
}
int hip_refuse(qpgpu_ctx *ctx, char *err, hipError_t e, const char *what) {
    const int rc = e == hipErrorOutOfMemory ? ctx->fail(QPGPU_ENOMEM, std::string(what) + ": out of device memory") : ctx->hip_fail(e, what);
    if (err) std::snprintf(err, QPGPU_LEAF_ERR_CAP, "%s", ctx->err.c_str());
    return rc;
}
#define ZK_HIP(ctx, err, call, what) do { hipError_t _e = (call); if (_e != hipSuccess) return hip_refuse((ctx), (err), _e, (what)); } while (0)

// device -> host, synchronous on the context's stream
int read_nodes(qpgpu_ctx *ctx, void *dst, const void *d_src, size_t bytes, const char *what) {
    if (bytes == 0) return QPGPU_OK;
    ZK_HIP(ctx, nullptr, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream), what);
    ZK_HIP(ctx, nullptr, hipStreamSynchronize(ctx->stream), what);
    return QPGPU_OK;
}

// the body of both builds: `plan` holds `count` leaves in a layout for `capacity`
int build_tree(qpgpu_ctx *ctx, const void *leaves, const zk_tree::Plan &plan, uint64_t capacity, bool reserved, unsigned flags, qpgpu_zk_tree **out,
               char *err, const char *what) {
    const size_t count = (size_t)plan.count;
    int rc = ctx->ensure_p2_app();
    if (rc) { if (err) std::snprintf(err, QPGPU_LEAF_ERR_CAP, "%s", ctx->err.c_str()); return rc; }

    // the nodes, and behind them the word that names a refused leaf
    const size_t node_bytes = (size_t)plan.total() * zk_tree::NODE_BYTES;
    Scratch nodes, records;
    ZK_HIP(ctx, err, nodes.alloc(node_bytes + sizeof(Aux)), what);
    uint8_t *d_nodes = nodes.as<uint8_t>();
    uint32_t *d_bad = (uint32_t *)(d_nodes + node_bytes + offsetof(Aux, bad_leaf));
    ZK_HIP(ctx, err, hipMemsetAsync(d_bad, 0xFF, sizeof(uint32_t), ctx->stream), what);
    if (flags & zk_tree::FLAG_FROM_TRANSFERS) {
        ZK_HIP(ctx, err, records.alloc(count * zk_tree::LEAF_RECORD_BYTES), what);
        ZK_HIP(ctx, err, hipMemcpyAsync(records.p, leaves, count * zk_tree::LEAF_RECORD_BYTES, hipMemcpyHostToDevice, ctx->stream), what);
        ZK_HIP(ctx, err, zk_tree_leaf_hashes(records.as<uint8_t>(), count, d_nodes, ctx->d_p2_app, ctx->stream), what);
    } else {
        ZK_HIP(ctx, err, hipMemcpyAsync(d_nodes, leaves, count * zk_tree::NODE_BYTES, hipMemcpyHostToDevice, ctx->stream), what);
    }
    ctx->prof_begin("zk_tree_levels");
    const hipError_t e_levels = zk_tree_reduce(d_nodes, plan, d_bad, ctx->d_p2_app, ctx->stream);
    ctx->prof_end();
    ZK_HIP(ctx, err, e_levels, what);
    uint32_t bad = 0;
    ZK_HIP(ctx, err, hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, ctx->stream), what);
    ZK_HIP(ctx, err, hipStreamSynchronize(ctx->stream), what);
    if (bad != 0xFFFFFFFFu) {
        char why[96];
        std::snprintf(why, sizeof why, "leaf %u: hash bytes are noncanonical (a limb >= p)", bad);
        return refuse(ctx, err, QPGPU_EINVAL, what, why);
    }
    qpgpu_zk_tree *t = new (std::nothrow) qpgpu_zk_tree;
    if (!t) return refuse(ctx, err, QPGPU_ENOMEM, what, "out of host memory");
    t->ctx = ctx; t->plan = plan; t->capacity = capacity; t->reserved = reserved; t->d_nodes = d_nodes;
    nodes.p = nullptr;               // owned by the handle from here, and listed with the context (residue.hpp)
    ctx->mem.add(d_nodes, node_bytes + sizeof(Aux), residue::ZK_TREE, false);
    *out = t;
    return QPGPU_OK;
}

}  // namespace

extern "C" {

int qpgpu_zk_leaf_hash_batch(qpgpu_ctx *ctx, const qpgpu_zk_leaf *leaves, size_t count, uint8_t *out) {
    if (!ctx) return QPGPU_EINVAL;
    QP_DEV(ctx);
    static const char *const what = "zk_leaf_hash_batch";
    if (!leaves || !out) return refuse(ctx, nullptr, QPGPU_EINVAL, what, "null argument");
    if (count == 0 || count > zk_tree::MAX_LEAVES) return refuse(ctx, nullptr, QPGPU_EINVAL, what, "count must be 1 .. 2^24");
    int rc = ctx->ensure_p2_app();
    if (rc) return rc;
    Scratch rec, dig;
    ZK_HIP(ctx, nullptr, rec.alloc(count * zk_tree::LEAF_RECORD_BYTES), what);
    ZK_HIP(ctx, nullptr, dig.alloc(count * zk_tree::NODE_BYTES), what);
    ZK_HIP(ctx, nullptr, hipMemcpyAsync(rec.p, leaves, count * zk_tree::LEAF_RECORD_BYTES, hipMemcpyHostToDevice, ctx->stream), what);
    ZK_HIP(ctx, nullptr, zk_tree_leaf_hashes(rec.as<uint8_t>(), count, dig.as<uint8_t>(), ctx->d_p2_app, ctx->stream), what);
    return read_nodes(ctx, out, dig.p, count * zk_tree::NODE_BYTES, what);      // the sync also ends the kernel's use of both buffers
}

int qpgpu_zk_tree_build(qpgpu_ctx *ctx, const void *leaves, size_t count, unsigned depth, unsigned flags, qpgpu_zk_tree **out, char *err) {
    if (err) err[0] = 0;
    if (out) *out = nullptr;
    if (!ctx) { if (err) std::snprintf(err, QPGPU_LEAF_ERR_CAP, "zk_tree_build: null context"); return QPGPU_EINVAL; }
    QP_DEV(ctx);
    static const char *const what = "zk_tree_build";
    if (!leaves || !out) return refuse(ctx, err, QPGPU_EINVAL, what, "null argument");
    zk_tree::Plan plan;
    if (const char *why = zk_tree::make_plan(count, depth, flags, plan)) return refuse(ctx, err, QPGPU_EINVAL, what, why);
    return build_tree(ctx, leaves, plan, count, false, flags, out, err, what);
}

int qpgpu_zk_tree_build_reserved(qpgpu_ctx *ctx, const void *leaves, size_t count, size_t capacity, unsigned depth, unsigned flags,
                                 qpgpu_zk_tree **out, char *err) {
    if (err) err[0] = 0;
    if (out) *out = nullptr;
    if (!ctx) { if (err) std::snprintf(err, QPGPU_LEAF_ERR_CAP, "zk_tree_build_reserved: null context"); return QPGPU_EINVAL; }
    QP_DEV(ctx);
    static const char *const what = "zk_tree_build_reserved";
    if (!leaves || !out) return refuse(ctx, err, QPGPU_EINVAL, what, "null argument");
    zk_tree::Plan plan;
    if (const char *why = zk_tree::make_plan_reserved(count, capacity, depth, flags, plan)) return refuse(ctx, err, QPGPU_EINVAL, what, why);
    return build_tree(ctx, leaves, plan, capacity, true, flags, out, err, what);
}

void qpgpu_zk_tree_free(qpgpu_zk_tree *t) {
    if (!t) return;
    if (t->d_nodes && hipSetDevice(t->ctx->device) == hipSuccess) t->ctx->track_free(t->d_nodes);
    delete t;
}

unsigned qpgpu_zk_tree_depth(const qpgpu_zk_tree *t) { return t ? t->plan.depth : 0; }
size_t qpgpu_zk_tree_leaf_count(const qpgpu_zk_tree *t) { return t ? (size_t)t->plan.count : 0; }

int qpgpu_zk_tree_read_level(const qpgpu_zk_tree *t, unsigned level, size_t first, size_t n, uint8_t *out) {
    if (!t) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = t->ctx;
    QP_DEV(ctx);
    static const char *const what = "zk_tree_read_level";
    if (const char *why = zk_tree::check_range(t->plan, level, first, n)) return refuse(ctx, nullptr, QPGPU_EINVAL, what, why);
    if (!out && n) return refuse(ctx, nullptr, QPGPU_EINVAL, what, "null argument");
    return read_nodes(ctx, out, t->d_nodes + (t->plan.off[level] + first) * zk_tree::NODE_BYTES, n * zk_tree::NODE_BYTES, what);
}

int qpgpu_zk_tree_root(const qpgpu_zk_tree *t, uint8_t out[32]) {
    if (!t) return QPGPU_EINVAL;
    if (!out) return refuse(t->ctx, nullptr, QPGPU_EINVAL, "zk_tree_root", "null argument");
    return qpgpu_zk_tree_read_level(t, t->plan.depth, 0, 1, out);
}

int qpgpu_zk_tree_open(const qpgpu_zk_tree *t, const uint64_t *indices, size_t n, uint8_t *siblings_out, uint8_t *positions_out) {
    if (!t) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = t->ctx;
    QP_DEV(ctx);
    static const char *const what = "zk_tree_open";
    if (n == 0) return QPGPU_OK;
    if (!indices || !siblings_out || !positions_out) return refuse(ctx, nullptr, QPGPU_EINVAL, what, "null argument");
    uint64_t bad = 0;
    if (const char *why = zk_tree::check_open(t->plan, indices, n, &bad)) {
        char msg[96];
        if (std::strcmp(why, "leaf index out of range") == 0) std::snprintf(msg, sizeof msg, "entry %llu: %s", (unsigned long long)bad, why);
        else std::snprintf(msg, sizeof msg, "%s", why);
        return refuse(ctx, nullptr, QPGPU_EINVAL, what, msg);
    }
    const size_t rows = n * t->plan.depth;
    Scratch idx, sib, pos;
    ZK_HIP(ctx, nullptr, idx.alloc(n * sizeof(uint64_t)), what);
    ZK_HIP(ctx, nullptr, sib.alloc(rows * zk_tree::PATH_LEVEL_BYTES), what);
    ZK_HIP(ctx, nullptr, pos.alloc(rows), what);
    ZK_HIP(ctx, nullptr, hipMemcpyAsync(idx.p, indices, n * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream), what);
    ctx->prof_begin("zk_tree_open");
    const hipError_t e_open = zk_tree_open_paths(t->d_nodes, t->plan, idx.as<uint64_t>(), n, sib.as<uint8_t>(), pos.as<uint8_t>(), ctx->stream);
    ctx->prof_end();
    ZK_HIP(ctx, nullptr, e_open, what);
    ZK_HIP(ctx, nullptr, hipMemcpyAsync(siblings_out, sib.p, rows * zk_tree::PATH_LEVEL_BYTES, hipMemcpyDeviceToHost, ctx->stream), what);
    ZK_HIP(ctx, nullptr, hipMemcpyAsync(positions_out, pos.p, rows, hipMemcpyDeviceToHost, ctx->stream), what);
    ZK_HIP(ctx, nullptr, hipStreamSynchronize(ctx->stream), what);
    return QPGPU_OK;
}

size_t qpgpu_zk_tree_capacity(const qpgpu_zk_tree *t) { return t ? (size_t)t->capacity : 0; }

// The new leaves go into their level-0 slots, where they are invisible while the count stands, and are tested there; the rehash kernels
// do nothing once the refusal word is set; the count advances on the host after the one synchronisation. A refused append therefore
// leaves every live node as it was.
int qpgpu_zk_tree_append(qpgpu_zk_tree *t, const void *leaves, size_t k, unsigned flags, qpgpu_zk_snapshot *snap_out, char *err) {
    if (err) err[0] = 0;
    if (!t) { if (err) std::snprintf(err, QPGPU_LEAF_ERR_CAP, "zk_tree_append: null tree"); return QPGPU_EINVAL; }
    qpgpu_ctx *ctx = t->ctx;
    QP_DEV(ctx);
    static const char *const what = "zk_tree_append";
    if (const char *why = zk_tree::check_append(t->plan, t->capacity, t->reserved, k, flags)) return refuse(ctx, err, QPGPU_EINVAL, what, why);
    if (!leaves) return refuse(ctx, err, QPGPU_EINVAL, what, "null argument");
    const uint64_t n_old = t->plan.count;
    zk_tree::Plan grown;
    if (const char *why = zk_tree::make_plan_reserved(n_old + k, t->capacity, t->plan.depth, flags, grown)) return refuse(ctx, err, QPGPU_EINVAL, what, why);

    uint8_t *d_aux = t->d_aux(), *d_new = t->d_nodes + n_old * zk_tree::NODE_BYTES;
    uint32_t *d_bad = (uint32_t *)(d_aux + offsetof(Aux, bad_leaf));
    Scratch records;
    ZK_HIP(ctx, err, hipMemsetAsync(d_bad, 0xFF, sizeof(uint32_t), ctx->stream), what);
    if (flags & zk_tree::FLAG_FROM_TRANSFERS) {          // permutation outputs: canonical by construction
        ZK_HIP(ctx, err, records.alloc(k * zk_tree::LEAF_RECORD_BYTES), what);
        ZK_HIP(ctx, err, hipMemcpyAsync(records.p, leaves, k * zk_tree::LEAF_RECORD_BYTES, hipMemcpyHostToDevice, ctx->stream), what);
        ZK_HIP(ctx, err, zk_tree_leaf_hashes(records.as<uint8_t>(), k, d_new, ctx->d_p2_app, ctx->stream), what);
    } else {
        ZK_HIP(ctx, err, hipMemcpyAsync(d_new, leaves, k * zk_tree::NODE_BYTES, hipMemcpyHostToDevice, ctx->stream), what);
    }
    ctx->prof_begin("zk_tree_append");
    hipError_t e = (flags & zk_tree::FLAG_FROM_TRANSFERS) ? hipSuccess : zk_tree_check_leaves(t->d_nodes, grown, n_old, k, d_bad, ctx->stream);
    if (e == hipSuccess) e = zk_tree_rehash(t->d_nodes, grown, n_old, d_bad, d_aux + offsetof(Aux, snap), ctx->d_p2_app, ctx->stream);
    ctx->prof_end();
    ZK_HIP(ctx, err, e, what);
    Aux aux;
    ZK_HIP(ctx, err, hipMemcpyAsync(&aux, d_aux, sizeof aux, hipMemcpyDeviceToHost, ctx->stream), what);
    ZK_HIP(ctx, err, hipStreamSynchronize(ctx->stream), what);      // also ends the kernel's use of `records`
    if (aux.bad_leaf != 0xFFFFFFFFu) {
        char why[96];
        std::snprintf(why, sizeof why, "leaf %u: hash bytes are noncanonical (a limb >= p)", aux.bad_leaf);
        return refuse(ctx, err, QPGPU_EINVAL, what, why);
    }
    t->plan = grown;
    if (snap_out) {
        std::memset(snap_out, 0, sizeof *snap_out);
        snap_out->count = grown.count; snap_out->depth = grown.depth;
        std::memcpy(snap_out->last, aux.snap, sizeof aux.snap);
    }
    return QPGPU_OK;
}

int qpgpu_zk_tree_snapshot(const qpgpu_zk_tree *t, qpgpu_zk_snapshot *out) {
    if (!t) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = t->ctx;
    QP_DEV(ctx);
    static const char *const what = "zk_tree_snapshot";
    if (!out) return refuse(ctx, nullptr, QPGPU_EINVAL, what, "null argument");
    uint8_t *d_snap = t->d_aux() + offsetof(Aux, snap);
    ZK_HIP(ctx, nullptr, zk_tree_gather_snapshot(t->d_nodes, t->plan, d_snap, ctx->stream), what);
    std::memset(out, 0, sizeof *out);
    out->count = t->plan.count; out->depth = t->plan.depth;
    return read_nodes(ctx, out->last, d_snap, zk_tree::SNAPSHOT_NODES_BYTES, what);
}

int qpgpu_zk_tree_open_at(const qpgpu_zk_tree *t, const qpgpu_zk_snapshot *snap, const uint64_t *indices, size_t n, uint8_t *siblings_out,
                          uint8_t *positions_out) {
    if (!t) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = t->ctx;
    QP_DEV(ctx);
    static const char *const what = "zk_tree_open_at";
    if (!snap || (n && (!indices || !siblings_out || !positions_out))) return refuse(ctx, nullptr, QPGPU_EINVAL, what, "null argument");
    uint64_t bad = 0;
    if (const char *why = zk_tree::check_open_at(t->plan, snap->count, snap->depth, indices, n, &bad)) {
        char msg[96];
        if (std::strcmp(why, "leaf index out of range") == 0) std::snprintf(msg, sizeof msg, "entry %llu: %s", (unsigned long long)bad, why);
        else std::snprintf(msg, sizeof msg, "%s", why);
        return refuse(ctx, nullptr, QPGPU_EINVAL, what, msg);
    }
    if (n == 0) return QPGPU_OK;
    zk_tree::Snapshot at;
    std::memcpy(&at, snap, sizeof at);
    const size_t rows = n * t->plan.depth;
    Scratch idx, sib, pos;
    ZK_HIP(ctx, nullptr, idx.alloc(n * sizeof(uint64_t)), what);
    ZK_HIP(ctx, nullptr, sib.alloc(rows * zk_tree::PATH_LEVEL_BYTES), what);
    ZK_HIP(ctx, nullptr, pos.alloc(rows), what);
    ZK_HIP(ctx, nullptr, hipMemcpyAsync(idx.p, indices, n * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream), what);
    ctx->prof_begin("zk_tree_open_at");
    const hipError_t e_open = zk_tree_open_paths_at(t->d_nodes, t->plan, at, idx.as<uint64_t>(), n, sib.as<uint8_t>(), pos.as<uint8_t>(), ctx->stream);
    ctx->prof_end();
    ZK_HIP(ctx, nullptr, e_open, what);
    ZK_HIP(ctx, nullptr, hipMemcpyAsync(siblings_out, sib.p, rows * zk_tree::PATH_LEVEL_BYTES, hipMemcpyDeviceToHost, ctx->stream), what);
    ZK_HIP(ctx, nullptr, hipMemcpyAsync(positions_out, pos.p, rows, hipMemcpyDeviceToHost, ctx->stream), what);
    ZK_HIP(ctx, nullptr, hipStreamSynchronize(ctx->stream), what);
    return QPGPU_OK;
}

// ---- the tree at earlier counts out of the tree alone, and reorgs (zk_tree.hpp: last_node; zk_snapshots_at_kernel) ----

int qpgpu_zk_tree_snapshots_at(const qpgpu_zk_tree *t, const uint64_t *counts, size_t m, qpgpu_zk_snapshot *out) {
    if (!t) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = t->ctx;
    QP_DEV(ctx);
    static const char *const what = "zk_tree_snapshots_at";
    if (m == 0) return QPGPU_OK;
    if (!counts || !out) return refuse(ctx, nullptr, QPGPU_EINVAL, what, "null argument");
    uint64_t bad = 0;
    if (const char *why = zk_tree::check_counts(t->plan, counts, m, &bad)) {
        char msg[96];
        if (std::strncmp(why, "count ", 6) == 0) std::snprintf(msg, sizeof msg, "entry %llu: %s", (unsigned long long)bad, why);
        else std::snprintf(msg, sizeof msg, "%s", why);
        return refuse(ctx, nullptr, QPGPU_EINVAL, what, msg);
    }
    Scratch cnt, snaps;
    ZK_HIP(ctx, nullptr, cnt.alloc(m * sizeof(uint64_t)), what);
    ZK_HIP(ctx, nullptr, snaps.alloc(m * sizeof(zk_tree::Snapshot)), what);
    ZK_HIP(ctx, nullptr, hipMemcpyAsync(cnt.p, counts, m * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream), what);
    ctx->prof_begin("zk_tree_snapshots_at");
    const hipError_t e = zk_tree_derive_snapshots(t->d_nodes, t->plan, cnt.as<uint64_t>(), m, snaps.as<zk_tree::Snapshot>(), ctx->d_p2_app, ctx->stream);
    ctx->prof_end();
    ZK_HIP(ctx, nullptr, e, what);
    return read_nodes(ctx, out, snaps.p, m * sizeof(zk_tree::Snapshot), what);      // the sync also ends the kernel's use of both buffers
}

int qpgpu_zk_tree_snapshot_check(const qpgpu_zk_tree *t, const qpgpu_zk_snapshot *snap) {
    if (!t) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = t->ctx;
    QP_DEV(ctx);
    static const char *const what = "zk_tree_snapshot_check";
    if (!snap) return refuse(ctx, nullptr, QPGPU_EINVAL, what, "null argument");
    if (const char *why = zk_tree::check_open_at(t->plan, snap->count, snap->depth, nullptr, 0, nullptr)) return refuse(ctx, nullptr, QPGPU_EINVAL, what, why);
    qpgpu_zk_snapshot own;
    const uint64_t count = snap->count;
    if (int rc = qpgpu_zk_tree_snapshots_at(t, &count, 1, &own)) return rc;
    for (unsigned l = 1; l <= t->plan.depth; l++)
        if (std::memcmp(own.last[l - 1], snap->last[l - 1], zk_tree::NODE_BYTES) != 0) {
            char msg[96];
            std::snprintf(msg, sizeof msg, "snapshot differs from the tree's at count %llu: the last node of level %u", (unsigned long long)count, l);
            return refuse(ctx, nullptr, QPGPU_EINVAL, what, msg);
        }
    if (std::memcmp(&own, snap, sizeof own) != 0)
        return refuse(ctx, nullptr, QPGPU_EINVAL, what, "snapshot differs from the tree's: the reserved word or an entry above the depth is not zero");
    return QPGPU_OK;
}

int qpgpu_zk_tree_open_at_counts(const qpgpu_zk_tree *t, const uint64_t *counts, const uint64_t *indices, size_t n, uint8_t *siblings_out,
                                 uint8_t *positions_out, uint8_t *roots_out) {
    if (!t) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = t->ctx;
    QP_DEV(ctx);
    static const char *const what = "zk_tree_open_at_counts";
    if (n == 0) return QPGPU_OK;
    if (!counts || !indices || !siblings_out || !positions_out) return refuse(ctx, nullptr, QPGPU_EINVAL, what, "null argument");
    uint64_t bad = 0;
    if (const char *why = zk_tree::check_open_at_counts(t->plan, counts, indices, n, &bad)) {
        char msg[96];
        if (std::strncmp(why, "too many", 8) != 0) std::snprintf(msg, sizeof msg, "entry %llu: %s", (unsigned long long)bad, why);
        else std::snprintf(msg, sizeof msg, "%s", why);
        return refuse(ctx, nullptr, QPGPU_EINVAL, what, msg);
    }
    // one upload: the leaf indices, the distinct counts (sorted), and for every path the place of its count among them
    std::vector<uint64_t> distinct;
    std::vector<uint8_t> up;
    size_t m = 0;
    try {
        distinct.assign(counts, counts + n);
        std::sort(distinct.begin(), distinct.end());
        distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
        m = distinct.size();
        up.resize((n + m) * sizeof(uint64_t) + n * sizeof(uint32_t));
    } catch (const std::bad_alloc &) {
        return refuse(ctx, nullptr, QPGPU_ENOMEM, what, "out of host memory");
    }
    const size_t off_counts = n * sizeof(uint64_t), off_snap_of = (n + m) * sizeof(uint64_t);
    std::memcpy(up.data(), indices, n * sizeof(uint64_t));
    std::memcpy(up.data() + off_counts, distinct.data(), m * sizeof(uint64_t));
    uint32_t *snap_of = (uint32_t *)(up.data() + off_snap_of);
    for (size_t i = 0; i < n; i++) snap_of[i] = (uint32_t)(std::lower_bound(distinct.begin(), distinct.end(), counts[i]) - distinct.begin());

    const size_t rows = n * t->plan.depth;
    Scratch in, snaps, sib, pos, roots;
    ZK_HIP(ctx, nullptr, in.alloc(up.size()), what);
    ZK_HIP(ctx, nullptr, snaps.alloc(m * sizeof(zk_tree::Snapshot)), what);
    ZK_HIP(ctx, nullptr, sib.alloc(rows * zk_tree::PATH_LEVEL_BYTES), what);
    ZK_HIP(ctx, nullptr, pos.alloc(rows), what);
    if (roots_out) ZK_HIP(ctx, nullptr, roots.alloc(n * zk_tree::NODE_BYTES), what);
    ZK_HIP(ctx, nullptr, hipMemcpyAsync(in.p, up.data(), up.size(), hipMemcpyHostToDevice, ctx->stream), what);
    const uint8_t *d_in = in.as<uint8_t>();
    ctx->prof_begin("zk_tree_open_at_counts");
    hipError_t e = zk_tree_derive_snapshots(t->d_nodes, t->plan, (const uint64_t *)(d_in + off_counts), m, snaps.as<zk_tree::Snapshot>(), ctx->d_p2_app,
                                            ctx->stream);
    if (e == hipSuccess)
        e = zk_tree_open_paths_at_many(t->d_nodes, t->plan, snaps.as<zk_tree::Snapshot>(), m, (const uint32_t *)(d_in + off_snap_of), (const uint64_t *)d_in,
                                       n, sib.as<uint8_t>(), pos.as<uint8_t>(), roots.as<uint8_t>(), ctx->stream);
    ctx->prof_end();
    ZK_HIP(ctx, nullptr, e, what);
    ZK_HIP(ctx, nullptr, hipMemcpyAsync(siblings_out, sib.p, rows * zk_tree::PATH_LEVEL_BYTES, hipMemcpyDeviceToHost, ctx->stream), what);
    ZK_HIP(ctx, nullptr, hipMemcpyAsync(positions_out, pos.p, rows, hipMemcpyDeviceToHost, ctx->stream), what);
    if (roots_out) ZK_HIP(ctx, nullptr, hipMemcpyAsync(roots_out, roots.p, n * zk_tree::NODE_BYTES, hipMemcpyDeviceToHost, ctx->stream), what);
    ZK_HIP(ctx, nullptr, hipStreamSynchronize(ctx->stream), what);
    return QPGPU_OK;
}

// The snapshot at n is derived from the nodes as they stand, then written over the last node of every level at the sizes of n: every
// other node of those sizes is resident and unchanged since the tree had n leaves, so the tree is the one built from its first n leaves.
// What lies beyond the new sizes stays in memory, unreachable: every read is bounded by the plan's sizes.
int qpgpu_zk_tree_truncate(qpgpu_zk_tree *t, size_t n, qpgpu_zk_snapshot *snap_out, char *err) {
    if (err) err[0] = 0;
    if (!t) { if (err) std::snprintf(err, QPGPU_LEAF_ERR_CAP, "zk_tree_truncate: null tree"); return QPGPU_EINVAL; }
    qpgpu_ctx *ctx = t->ctx;
    QP_DEV(ctx);
    static const char *const what = "zk_tree_truncate";
    if (const char *why = zk_tree::check_truncate(t->plan, n)) return refuse(ctx, err, QPGPU_EINVAL, what, why);
    zk_tree::Plan cut;
    if (const char *why = zk_tree::make_plan_reserved(n, t->capacity, t->plan.depth, 0, cut)) return refuse(ctx, err, QPGPU_EINVAL, what, why);
    const uint64_t count = n;
    Scratch cnt, snap;
    ZK_HIP(ctx, err, cnt.alloc(sizeof count), what);
    ZK_HIP(ctx, err, snap.alloc(sizeof(zk_tree::Snapshot)), what);
    ZK_HIP(ctx, err, hipMemcpyAsync(cnt.p, &count, sizeof count, hipMemcpyHostToDevice, ctx->stream), what);
    ctx->prof_begin("zk_tree_truncate");
    hipError_t e = zk_tree_derive_snapshots(t->d_nodes, t->plan, cnt.as<uint64_t>(), 1, snap.as<zk_tree::Snapshot>(), ctx->d_p2_app, ctx->stream);
    if (e == hipSuccess) e = zk_tree_place_snapshot(t->d_nodes, cut, snap.as<zk_tree::Snapshot>(), t->d_aux() + offsetof(Aux, snap), ctx->stream);
    ctx->prof_end();
    ZK_HIP(ctx, err, e, what);
    qpgpu_zk_snapshot at;
    ZK_HIP(ctx, err, hipMemcpyAsync(&at, snap.p, sizeof at, hipMemcpyDeviceToHost, ctx->stream), what);
    ZK_HIP(ctx, err, hipStreamSynchronize(ctx->stream), what);      // also ends the kernels' use of both buffers
    t->plan = cut;
    if (snap_out) *snap_out = at;
    return QPGPU_OK;
}

}  // extern "C"
