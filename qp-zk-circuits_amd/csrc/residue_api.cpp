// residue_api.cpp — the residue registry (residue.hpp) bound to HIP: tracked allocation and release for a context, the scan backend
// over residue_kernels.hip, and the C ABI of include/qpgpu.h ("secret residue audit").
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include "ctx.hpp"
#include "residue_kernels.hpp"

namespace {

int scan_backend(void *user, const residue::Entry &e, const uint64_t *needles, size_t n, uint64_t *count, residue::Found *found, size_t cap, size_t *filled, std::string *why) {
    qpgpu_ctx *ctx = (qpgpu_ctx *)user;
    const uint64_t words = e.bytes / 8;
    if (e.pinned) {      // host memory: the device may still be writing it, so wait first
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) { *why = "residue scan: hipStreamSynchronize failed"; return QPGPU_EDEVICE; }
        const volatile uint64_t *w = (const volatile uint64_t *)e.ptr;
        uint64_t c = 0;
        for (uint64_t i = 0; i < words; i++) {
            const uint64_t v = w[i];
            for (size_t k = 0; k < n; k++)
                if (v == needles[k]) { if (c < cap) found[c] = residue::Found{v, i}; c++; break; }
        }
        *count += c;
        *filled = (size_t)std::min<uint64_t>(c, cap);
        return QPGPU_OK;
    }
    hipError_t err = hipSuccess;
    if (!ctx->d_residue) err = hipMalloc((void **)&ctx->d_residue, sizeof(ResidueResult));
    if (err == hipSuccess) err = hipMemsetAsync(ctx->d_residue, 0, sizeof(ResidueResult), ctx->stream);
    ResidueNeedles nd{};
    for (size_t k = 0; k < n; k++) nd.v[k] = needles[k];
    nd.n = (uint32_t)n;
    ctx->prof_begin("residue_scan");       // qpgpu_profile_read("residue_scan"): the kernel's time alone, for its rate
    if (err == hipSuccess) err = rk_scan((const uint64_t *)e.ptr, words, nd, ctx->d_residue, ctx->stream);
    ctx->prof_end();
    ResidueResult res;
    if (err == hipSuccess) err = hipMemcpyAsync(&res, ctx->d_residue, sizeof res, hipMemcpyDeviceToHost, ctx->stream);
    // what the scan found goes again at once: the result block is the one buffer the registry does not list
    if (err == hipSuccess) err = hipMemsetAsync(ctx->d_residue, 0, sizeof(ResidueResult), ctx->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
    volatile uint64_t *z = nd.v;
    for (size_t k = 0; k < QPGPU_RESIDUE_MAX_NEEDLES; k++) z[k] = 0;
    if (err != hipSuccess) { *why = std::string("residue scan: ") + hipGetErrorString(err); return QPGPU_EDEVICE; }
    const uint64_t keep = std::min<uint64_t>(std::min<uint64_t>(res.count, RESIDUE_DEV_CAP), cap);
    for (uint64_t i = 0; i < keep; i++) found[i] = residue::Found{res.found[i].word, res.found[i].offset_words};
    *count += res.count;
    *filled = (size_t)keep;
    std::memset(&res, 0, sizeof res);
    return QPGPU_OK;
}

void release_backend(void *, const residue::Entry &e) {
    if (e.pinned) (void)hipHostFree(e.ptr);
    else (void)hipFree(e.ptr);
}

}  // namespace

// once, by qpgpu_ctx_create, before the context is handed out
void qpgpu_ctx::bind_residue_backend() {
    mem.backend.user = this;
    mem.backend.scan = scan_backend;
    mem.backend.release = release_backend;
}

hipError_t qpgpu_ctx::track_malloc(void **p, size_t bytes, uint32_t region) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) mem.add(*p, bytes, region, false);
    return e;
}
hipError_t qpgpu_ctx::track_host_malloc(void **p, size_t bytes, uint32_t region) {
    const hipError_t e = hipHostMalloc(p, bytes, hipHostMallocDefault);
    if (e == hipSuccess) mem.add(*p, bytes, region, true);
    return e;
}
void qpgpu_ctx::track_free(void *p) {
    if (!p) return;
    (void)mem.release(p);
}
void qpgpu_ctx::scrub_scratch() {
    if (scratch) (void)hipMemsetAsync(scratch, 0, scratch_bytes, stream);
}
void qpgpu_ctx::scrub_pinned() {
    if (h_pin) std::memset(h_pin, 0, h_pin_bytes);
}

extern "C" {

const char *qpgpu_residue_region_name(uint32_t region) { return residue::region_name(region); }

int qpgpu_ctx_residue_scan(qpgpu_ctx *ctx, const uint64_t *needles, size_t n_needles, uint64_t region_mask,
                           uint64_t *hits, qpgpu_residue_hit *first_hits, size_t cap, uint64_t *bytes_scanned) {
    if (!ctx) return QPGPU_EINVAL;
    QP_DEV(ctx);
    if (cap && !first_hits) return ctx->fail(QPGPU_EINVAL, "residue_scan: cap without a first_hits array");
    residue::Totals t;
    const int rc = ctx->mem.scan(needles, n_needles, region_mask, cap, t);
    if (rc) return ctx->fail(rc, ctx->mem.err);
    if (hits) *hits = t.hits;
    if (bytes_scanned) *bytes_scanned = t.bytes;
    for (size_t i = 0; i < t.first.size(); i++) first_hits[i] = t.first[i];
    return QPGPU_OK;
}

int qpgpu_ctx_residue_audit_begin(qpgpu_ctx *ctx, const uint64_t *needles, size_t n_needles) {
    if (!ctx) return QPGPU_EINVAL;
    const int rc = ctx->mem.audit_begin(needles, n_needles);
    return rc ? ctx->fail(rc, ctx->mem.err) : QPGPU_OK;
}

int qpgpu_ctx_residue_audit_end(qpgpu_ctx *ctx, uint64_t *hits, qpgpu_residue_hit *first_hits, size_t cap, uint64_t *buffers_released) {
    if (!ctx) return QPGPU_EINVAL;
    if (cap && !first_hits) return ctx->fail(QPGPU_EINVAL, "residue_audit_end: cap without a first_hits array");
    residue::Totals t;
    const int rc = ctx->mem.audit_end(cap, t, buffers_released);
    if (rc) return ctx->fail(rc, ctx->mem.err);
    if (hits) *hits = t.hits;
    for (size_t i = 0; i < t.first.size(); i++) first_hits[i] = t.first[i];
    return QPGPU_OK;
}

}  // extern "C"
