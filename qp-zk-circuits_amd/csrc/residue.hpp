// residue.hpp — the registry of device and pinned memory a context owns, and the secret-residue scan over it.
//
// The counterpart of the reference's allocator test (wormhole/circuit/tests/heap_zeroization.rs: a custom allocator scans every
// freed block for the secret): every hipMalloc / hipHostMalloc made on behalf of a qpgpu_ctx is listed here with its size and
// a region, a scan walks the list looking for caller-supplied 64-bit needle words, and an audit scans every buffer once more
// right before the library frees it. This file and residue.cpp are plain host C++ without a HIP call: how a buffer is scanned
// and freed is injected (Backend), so that a stand-alone program drives the bookkeeping over host memory
// (tests/native/residue_registry_main.cpp); residue_api.cpp injects the device kernel of residue_kernels.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/qpgpu.h"

namespace residue {

enum Region : uint32_t {
    CIRCUIT_SETUP = 0,     // public: constants, sigmas, gate and subgroup tables of a loaded circuit or stage plan
    CIRCUIT_WORKSPACE,     // per-proof workspace of a circuit handle, its pinned staging ring included
    WITNESS_PLAN,          // stage s1 plan: instruction lists (public) and the public-input value / hash / error buffers
    PARTIAL_WITNESS,       // prepared PartialWitness assignments: indices, values, ChaCha keys of device-drawn cells
    CTX_SCRATCH,           // transform scratch of the context
    CTX_PINNED,            // the context's pinned bounce / read-back buffer
    ORACLE,                // qpgpu_oracle blocks
    STAGE_PLAN,            // qpgpu_stage_plan workspace and its pinned ring
    FRI_SESSION,           // FRI workspace of qpgpu_fri_prove / qpgpu_fri_session and its pinned ring
    POOL_WITNESS,          // a pool worker's resident witness matrices
    VERIFY_STAGING,        // batch verification staging (proofs: public)
    ZK_TREE,               // the chain's ZK Merkle tree (public)
    TABLES,                // twiddle / coset tables and hasher parameter blocks of the context (public)
    NUM_REGIONS
};
const char *region_name(uint32_t region);      // NULL past the end
// region_mask 0: everything that can hold witness-derived words
constexpr uint64_t ALL_REGIONS = (1ull << NUM_REGIONS) - 1;
constexpr uint64_t DEFAULT_MASK = ALL_REGIONS & ~((1ull << CIRCUIT_SETUP) | (1ull << TABLES) | (1ull << ZK_TREE) | (1ull << VERIFY_STAGING));

struct Entry { void *ptr; size_t bytes; uint32_t region; bool pinned; };
struct Found { uint64_t word, offset_words; };

struct Backend {
    void *user = nullptr;
    // looks for any of needles[0..n) among the bytes / 8 aligned 64-bit words of e; *count += matches; up to `cap` of them (of
    // this buffer) go to found[], *filled says how many (a backend may record fewer than cap: the device kernel keeps 64 per
    // buffer). Returns 0, or nonzero with *why set.
    int (*scan)(void *user, const Entry &e, const uint64_t *needles, size_t n, uint64_t *count, Found *found, size_t cap, size_t *filled, std::string *why) = nullptr;
    void (*release)(void *user, const Entry &e) = nullptr;     // frees e.ptr
};

struct Totals {
    uint64_t hits = 0, bytes = 0;
    std::vector<qpgpu_residue_hit> first;     // at most the cap the scan was given
};

class Registry {
public:
    static constexpr size_t AUDIT_CAP = 64;   // hits an audit keeps in full
    Backend backend;
    std::string err;

    void add(void *ptr, size_t bytes, uint32_t region, bool pinned);
    // the audit's scan when one is open, then backend.release, then the entry goes. A pointer the registry does not list is
    // released as a device buffer all the same (false is returned): nothing the library frees may leak because it was not tracked.
    bool release(void *ptr);
    // forget an entry without freeing it (a buffer whose ownership passes elsewhere); false: not listed
    bool forget(void *ptr);
    size_t size() const;
    uint64_t tracked_bytes(uint64_t region_mask) const;
    bool find(const void *ptr, Entry *out) const;

    // 0, or QPGPU_EINVAL / the backend's code with err set
    static int check_needles(const uint64_t *needles, size_t n, std::string *why);
    int scan(const uint64_t *needles, size_t n, uint64_t region_mask, size_t cap, Totals &out);
    int audit_begin(const uint64_t *needles, size_t n);
    int audit_end(size_t cap, Totals &out, uint64_t *buffers_released);
    bool auditing() const { return audit_on_; }

private:
    int scan_entry(const Entry &e, const uint64_t *needles, size_t n, size_t cap, Totals &out);
    mutable std::mutex mu_;
    std::vector<Entry> entries_;
    bool audit_on_ = false;
    std::vector<uint64_t> audit_needles_;
    Totals audit_;
    uint64_t audit_released_ = 0;
};

}  // namespace residue
