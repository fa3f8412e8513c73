// residue.cpp — bookkeeping of the residue registry (residue.hpp). No HIP call in this file.
#include "residue.hpp"
#include <algorithm>

namespace residue {

const char *region_name(uint32_t region) {
    static const char *const names[NUM_REGIONS] = {
        "circuit-setup", "circuit-workspace", "witness-plan", "partial-witness", "ctx-scratch", "ctx-pinned", "oracle",
        "stage-plan", "fri-session", "pool-witness", "verify-staging", "zk-tree", "tables"};
    return region < NUM_REGIONS ? names[region] : nullptr;
}

void Registry::add(void *ptr, size_t bytes, uint32_t region, bool pinned) {
    if (!ptr) return;
    std::lock_guard<std::mutex> lk(mu_);
    entries_.push_back(Entry{ptr, bytes, region, pinned});
}

size_t Registry::size() const {
    std::lock_guard<std::mutex> lk(mu_);
    return entries_.size();
}

bool Registry::find(const void *ptr, Entry *out) const {
    std::lock_guard<std::mutex> lk(mu_);
    for (const Entry &e : entries_) if (e.ptr == ptr) { if (out) *out = e; return true; }
    return false;
}

bool Registry::forget(void *ptr) {
    std::lock_guard<std::mutex> lk(mu_);
    for (size_t i = 0; i < entries_.size(); i++)
        if (entries_[i].ptr == ptr) { entries_.erase(entries_.begin() + (ptrdiff_t)i); return true; }
    return false;
}

bool Registry::release(void *ptr) {
    if (!ptr) return false;
    Entry e{ptr, 0, NUM_REGIONS, false};
    const bool listed = find(ptr, &e);
    if (listed && audit_on_) {
        // after whatever scrub the release path performed, before the allocator gets the memory back. A scan that fails
        // (device error) is remembered in err; the buffer is released regardless.
        (void)scan_entry(e, audit_needles_.data(), audit_needles_.size(), AUDIT_CAP, audit_);
        audit_released_++;
    }
    if (backend.release) backend.release(backend.user, e);
    if (listed) forget(ptr);
    return listed;
}

uint64_t Registry::tracked_bytes(uint64_t region_mask) const {
    std::lock_guard<std::mutex> lk(mu_);
    uint64_t total = 0;
    for (const Entry &e : entries_) if (region_mask >> e.region & 1) total += e.bytes;
    return total;
}

int Registry::check_needles(const uint64_t *needles, size_t n, std::string *why) {
    if (!needles || n == 0 || n > QPGPU_RESIDUE_MAX_NEEDLES) {
        *why = "residue: the needle count must be 1.." + std::to_string(QPGPU_RESIDUE_MAX_NEEDLES) + " (got " + std::to_string(n) + ")";
        return QPGPU_EINVAL;
    }
    for (size_t i = 0; i < n; i++)
        if (needles[i] < (1ull << 32)) {
            *why = "residue: needle " + std::to_string(i) + " is below 2^32 (values of that size occur in tables by chance; a sensitive 64-bit word does not)";
            return QPGPU_EINVAL;
        }
    return QPGPU_OK;
}

int Registry::scan_entry(const Entry &e, const uint64_t *needles, size_t n, size_t cap, Totals &out) {
    if (!backend.scan) { err = "residue: no scan backend"; return QPGPU_EINVAL; }
    const size_t room = cap > out.first.size() ? cap - out.first.size() : 0;
    std::vector<Found> found(room);
    uint64_t count = 0;
    size_t filled = 0;
    std::string why;
    const int rc = backend.scan(backend.user, e, needles, n, &count, found.data(), room, &filled, &why);
    if (rc) { err = why; return rc; }
    out.hits += count;
    out.bytes += e.bytes;
    const size_t keep = std::min(filled, room);      // never more than the backend wrote
    for (size_t i = 0; i < keep; i++)
        out.first.push_back(qpgpu_residue_hit{found[i].word, e.region, e.pinned ? 1u : 0u, found[i].offset_words, (uint64_t)e.bytes});
    return QPGPU_OK;
}

int Registry::scan(const uint64_t *needles, size_t n, uint64_t region_mask, size_t cap, Totals &out) {
    out = Totals();
    int rc = check_needles(needles, n, &err);
    if (rc) return rc;
    if (region_mask & ~ALL_REGIONS) { err = "residue: region_mask names a region beyond the last one (" + std::string(region_name(NUM_REGIONS - 1)) + ")"; return QPGPU_EINVAL; }
    if (region_mask == 0) region_mask = DEFAULT_MASK;
    std::vector<Entry> todo;
    {
        std::lock_guard<std::mutex> lk(mu_);
        for (const Entry &e : entries_) if (region_mask >> e.region & 1) todo.push_back(e);
    }
    for (const Entry &e : todo) if ((rc = scan_entry(e, needles, n, cap, out)) != QPGPU_OK) return rc;
    return QPGPU_OK;
}

int Registry::audit_begin(const uint64_t *needles, size_t n) {
    const int rc = check_needles(needles, n, &err);
    if (rc) return rc;
    if (audit_on_) { err = "residue: an audit is already open on this context"; return QPGPU_EINVAL; }
    audit_needles_.assign(needles, needles + n);
    audit_ = Totals();
    audit_released_ = 0;
    audit_on_ = true;
    return QPGPU_OK;
}

int Registry::audit_end(size_t cap, Totals &out, uint64_t *buffers_released) {
    if (!audit_on_) { err = "residue: audit_end without audit_begin"; return QPGPU_EINVAL; }
    audit_on_ = false;
    out = audit_;
    if (out.first.size() > cap) out.first.resize(cap);
    if (buffers_released) *buffers_released = audit_released_;
    // the needles are sensitive words themselves
    volatile uint64_t *z = audit_needles_.data();
    for (size_t i = 0; i < audit_needles_.size(); i++) z[i] = 0;
    audit_needles_.clear();
    audit_ = Totals();
    return QPGPU_OK;
}

}  // namespace residue
