// quotient_map_check.cpp — the workgroup id -> (tile, proof) mapping of quotient_perm_gates_kernel (csrc/quotient_map.hpp, the code
// the kernel compiles) on the host, for every batch 1..33 and tile count 1..40, grouped and plain:
//   every (tile, proof) of the launch is the image of exactly one id of the grid, and the other ids (the padding of the last
//   group of eight tiles) map to nothing;
//   grouped: all workgroups of a tile have the same id modulo 8 (they run on one XCD) and lie within one group's 8 * batch ids.
// Stand-alone, built with -fsanitize=address,undefined and run by tests/test_quotient_map_host.py.
#include <cstdio>
#include <vector>
#include "quotient_map.hpp"

int main() {
    unsigned long failures = 0, launches = 0;
    for (int grouped = 0; grouped < 2; grouped++)
        for (uint32_t batch = 1; batch <= 33; batch++)
            for (uint32_t tiles = 1; tiles <= 40; tiles++) {
                const uint64_t grid = qmap::grid_size(tiles, batch, grouped != 0);
                std::vector<uint32_t> hits((size_t)tiles * batch, 0), residue(tiles, ~0u), first(tiles, ~0u);
                uint64_t padded = 0;
                for (uint64_t id = 0; id < grid; id++) {
                    const qmap::Place p = qmap::place((uint32_t)id, tiles, batch, grouped != 0);
                    if (!p.valid) { padded++; continue; }
                    if (p.tile >= tiles || p.proof >= batch) { failures++; continue; }
                    hits[(size_t)p.proof * tiles + p.tile]++;
                    if (grouped) {
                        if (residue[p.tile] == ~0u) { residue[p.tile] = (uint32_t)(id % qmap::XCDS); first[p.tile] = (uint32_t)id; }
                        if (residue[p.tile] != id % qmap::XCDS) failures++;
                        if (id - first[p.tile] >= (uint64_t)qmap::XCDS * batch) failures++;
                    }
                }
                for (uint32_t h : hits) if (h != 1) failures++;
                if (padded != grid - (uint64_t)tiles * batch) failures++;
                if (!grouped && padded) failures++;
                if (grouped && padded >= (uint64_t)qmap::XCDS * batch) failures++;
                launches++;
            }
    std::printf("quotient map: launches %lu, failures %lu\n", launches, failures);
    return failures ? 1 : 0;
}
