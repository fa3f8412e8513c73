// Drives the residue registry's bookkeeping (csrc/residue.hpp) over host memory: the scan and release operations the library
// injects from its HIP side are plain loops and free() here, so the whole of add / release / regrowth / region masks / hit
// recording / the needle rule / audit accounting runs under the address and undefined-behaviour sanitizers without a GPU.
// Built and run by tests/test_residue_host.py; prints one line per check and "residue registry: ok" at the end.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "residue.hpp"

using namespace residue;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static int scans = 0, frees = 0;
static const size_t BACKEND_CAP = 12;

static int host_scan(void *, const Entry &e, const uint64_t *needles, size_t n, uint64_t *count, Found *found, size_t cap, size_t *filled, std::string *why) {
    scans++;
    if (e.bytes == 24 * 8) { *why = "backend refuses this buffer"; return QPGPU_EDEVICE; }     // an injected device error
    const uint64_t *w = (const uint64_t *)e.ptr;
    uint64_t c = 0;
    for (size_t i = 0; i < e.bytes / 8; i++)
        for (size_t k = 0; k < n; k++)
            if (w[i] == needles[k]) { if (c < cap && c < BACKEND_CAP) found[c] = Found{w[i], i}; c++; break; }
    *count += c;
    // like the device kernel, this backend records a bounded number of hits per buffer however large cap is
    *filled = (size_t)(c < cap ? c : cap);
    if (*filled > BACKEND_CAP) *filled = BACKEND_CAP;
    return QPGPU_OK;
}
static void host_release(void *, const Entry &e) { frees++; std::free(e.ptr); }

static uint64_t *buffer(Registry &r, size_t words, uint32_t region, bool pinned, uint64_t fill = 7) {
    uint64_t *p = (uint64_t *)std::malloc(words * 8);
    for (size_t i = 0; i < words; i++) p[i] = fill + i;
    r.add(p, words * 8, region, pinned);
    return p;
}

int main() {
    const uint64_t S0 = 0xDEADBEEFCAFEF00Dull, S1 = 0x0123456789ABCDEFull;
    const uint64_t needles[2] = {S0, S1};
    Registry r;
    r.backend.scan = host_scan; r.backend.release = host_release;
    Totals t;

    // region names: the documented ones, NULL past the end
    const char *names[] = {"circuit-setup", "circuit-workspace", "witness-plan", "partial-witness", "ctx-scratch", "ctx-pinned", "oracle",
                           "stage-plan", "fri-session", "pool-witness", "verify-staging", "zk-tree", "tables"};
    CHECK(NUM_REGIONS == 13);
    for (uint32_t i = 0; i < NUM_REGIONS; i++) CHECK(std::strcmp(region_name(i), names[i]) == 0);
    CHECK(region_name(NUM_REGIONS) == nullptr && region_name(0xFFFFFFFFu) == nullptr);
    std::printf("names ok\n");

    // add, default mask, explicit masks, bytes_scanned
    uint64_t *setup = buffer(r, 16, CIRCUIT_SETUP, false), *work = buffer(r, 32, CIRCUIT_WORKSPACE, false);
    uint64_t *pin = buffer(r, 8, CTX_PINNED, true), *scratch = buffer(r, 10, CTX_SCRATCH, false);
    setup[3] = S0;                       // public regions are not in the default mask
    work[5] = S0; work[31] = S1; pin[0] = S1;
    CHECK(r.size() == 4 && r.tracked_bytes(ALL_REGIONS) == (16 + 32 + 8 + 10) * 8);
    CHECK(r.scan(needles, 2, 0, 8, t) == QPGPU_OK);
    CHECK(t.hits == 3 && t.bytes == (32 + 8 + 10) * 8 && t.bytes == r.tracked_bytes(DEFAULT_MASK) && t.first.size() == 3);
    CHECK(t.first[0].region == CIRCUIT_WORKSPACE && t.first[0].offset_words == 5 && t.first[0].word == S0 && t.first[0].pinned == 0 && t.first[0].alloc_bytes == 32 * 8);
    CHECK(t.first[1].offset_words == 31 && t.first[1].word == S1);
    CHECK(t.first[2].region == CTX_PINNED && t.first[2].pinned == 1 && t.first[2].offset_words == 0);
    CHECK(r.scan(needles, 2, 1ull << CIRCUIT_SETUP, 8, t) == QPGPU_OK && t.hits == 1 && t.bytes == 16 * 8 && t.first[0].region == CIRCUIT_SETUP);
    CHECK(r.scan(needles, 2, ALL_REGIONS, 8, t) == QPGPU_OK && t.hits == 4 && t.bytes == r.tracked_bytes(ALL_REGIONS));
    CHECK(r.scan(needles, 1, 1ull << CTX_SCRATCH, 8, t) == QPGPU_OK && t.hits == 0 && t.first.empty() && t.bytes == 80);
    std::printf("masks ok\n");

    // hits past cap are counted, not recorded; cap 0 records none
    for (size_t i = 0; i < 10; i++) scratch[i] = S1;
    CHECK(r.scan(needles, 2, 0, 4, t) == QPGPU_OK && t.hits == 13 && t.first.size() == 4);
    CHECK(t.first[2].region == CTX_PINNED && t.first[3].region == CTX_SCRATCH);   // registration order: workspace (2), pinned (1), then scratch
    CHECK(r.scan(needles, 2, 0, 0, t) == QPGPU_OK && t.hits == 13 && t.first.empty());
    CHECK(r.scan(needles, 2, 0, 100, t) == QPGPU_OK && t.hits == 13 && t.first.size() == 13);
    // a backend that records fewer hits than it counts: every hit is counted, no entry is made up for those it did not record
    uint64_t *wide = buffer(r, 40, FRI_SESSION, false);
    for (size_t i = 0; i < 40; i++) wide[i] = S0;
    CHECK(r.scan(needles, 2, 1ull << FRI_SESSION, 100, t) == QPGPU_OK && t.hits == 40 && t.first.size() == BACKEND_CAP);
    for (const qpgpu_residue_hit &h : t.first) CHECK(h.word == S0 && h.region == FRI_SESSION && h.alloc_bytes == 320);
    CHECK(r.release(wide) && frees == 1 && r.size() == 4);
    frees = 0;
    std::printf("cap ok\n");

    // the needle rule and the other refusals
    const uint64_t small[3] = {S0, 0xFFFFFFFFull, S1};
    CHECK(r.scan(small, 3, 0, 4, t) == QPGPU_EINVAL && r.err.find("needle 1") != std::string::npos && t.hits == 0);
    const uint64_t edge[1] = {1ull << 32};
    CHECK(r.scan(edge, 1, 0, 4, t) == QPGPU_OK);
    CHECK(r.scan(needles, 0, 0, 4, t) == QPGPU_EINVAL && r.scan(nullptr, 2, 0, 4, t) == QPGPU_EINVAL);
    std::vector<uint64_t> many(17, S0);
    CHECK(r.scan(many.data(), 17, 0, 4, t) == QPGPU_EINVAL && r.scan(many.data(), 16, 0, 4, t) == QPGPU_OK);
    CHECK(r.scan(needles, 2, 1ull << NUM_REGIONS, 4, t) == QPGPU_EINVAL && r.scan(needles, 2, 1ull << 63, 4, t) == QPGPU_EINVAL);
    std::printf("refusals ok\n");

    // audit: off by default (a release does not scan), begin/end accounting, regrowth
    CHECK(!r.auditing() && r.audit_end(4, t, nullptr) == QPGPU_EINVAL);
    int before = scans;
    CHECK(r.release(setup) && scans == before && frees == 1 && r.size() == 3);
    CHECK(r.audit_begin(small, 3) == QPGPU_EINVAL && !r.auditing());
    CHECK(r.audit_begin(needles, 2) == QPGPU_OK && r.auditing() && r.audit_begin(needles, 2) == QPGPU_EINVAL);
    // regrowth as ensure_scratch does it: scrub, release, a larger buffer under the same region
    std::memset(scratch, 0, 10 * 8);
    CHECK(r.release(scratch) && scans == before + 1);
    scratch = buffer(r, 20, CTX_SCRATCH, false);
    CHECK(r.size() == 3 && r.tracked_bytes(1ull << CTX_SCRATCH) == 160);
    // a release path that forgot its scrub: two needle words still there
    CHECK(r.release(work));
    // an entry the registry never saw is released all the same, and is not counted
    uint64_t *stray = (uint64_t *)std::malloc(64);
    CHECK(!r.release(stray) && frees == 4);
    CHECK(!r.release(nullptr) && frees == 4);
    uint64_t released = 0;
    CHECK(r.audit_end(1, t, &released) == QPGPU_OK && released == 2 && t.hits == 2 && t.first.size() == 1 && t.first[0].region == CIRCUIT_WORKSPACE);
    CHECK(!r.auditing() && r.audit_end(1, t, &released) == QPGPU_EINVAL);
    // a second audit starts from nothing
    CHECK(r.audit_begin(needles, 1) == QPGPU_OK);
    CHECK(r.audit_end(4, t, &released) == QPGPU_OK && released == 0 && t.hits == 0 && t.first.empty());
    std::printf("audit ok\n");

    // a backend error surfaces from scan, and an audited release still frees
    uint64_t *bad = buffer(r, 24, ORACLE, false);
    CHECK(r.scan(needles, 2, 1ull << ORACLE, 4, t) == QPGPU_EDEVICE && r.err == "backend refuses this buffer");
    CHECK(r.audit_begin(needles, 2) == QPGPU_OK);
    before = frees;
    CHECK(r.release(bad) && frees == before + 1);
    CHECK(r.audit_end(4, t, &released) == QPGPU_OK && released == 1 && t.hits == 0);
    // forget: the entry goes, the memory stays the caller's
    CHECK(r.forget(pin) && !r.forget(pin) && r.size() == 1);
    std::free(pin);
    Entry e;
    CHECK(r.find(scratch, &e) && e.bytes == 160 && e.region == CTX_SCRATCH && !r.find(pin, nullptr));
    CHECK(r.release(scratch) && r.size() == 0 && r.tracked_bytes(ALL_REGIONS) == 0);
    std::printf("backend ok\n");

    if (failures) { std::printf("residue registry: %d check(s) failed\n", failures); return 1; }
    std::printf("residue registry: ok\n");
    return 0;
}
