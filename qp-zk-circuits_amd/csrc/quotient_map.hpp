// quotient_map.hpp — workgroup id -> (tile of LDE slots, proof of the lockstep batch) for quotient_perm_gates_kernel's 1-D grid.
// Consecutive workgroup ids go to different XCDs (eight of them, each with an L2 of its own). The circuit-owned columns a tile
// reads (sigmas, selectors, constants, x and L_0 on the coset) are the same for every proof of the batch, so the `batch`
// workgroups of a tile get ids that are close together and equal modulo 8: one L2 then serves the tile's columns to all of its
// readers but the first. Tiles go in groups of eight, a group takes 8 * batch consecutive ids; the last group is padded to eight
// tiles, and the ids of its missing tiles (fewer than 8 * batch of them) map to nothing. The mapping changes placement only.
// Compiled by the kernel and by tools/host_checks/quotient_map_check.cpp.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define QMAP_HD __host__ __device__ __forceinline__
#else
#define QMAP_HD inline
#endif

namespace qmap {

constexpr uint32_t XCDS = 8;

struct Place { uint32_t tile, proof; bool valid; };

// ids the grid needs: grouped, whole groups of eight tiles; plain, tiles * batch (proof-major, the order of a (tiles, 1, batch) grid)
QMAP_HD uint64_t grid_size(uint32_t tiles, uint32_t batch, bool grouped) {
    return grouped ? (uint64_t)((tiles + XCDS - 1) / XCDS) * XCDS * batch : (uint64_t)tiles * batch;
}
QMAP_HD Place place(uint32_t id, uint32_t tiles, uint32_t batch, bool grouped) {
    Place p;
    if (grouped) {
        const uint32_t per_group = XCDS * batch, w = id % per_group;
        p.tile = XCDS * (id / per_group) + w % XCDS;
        p.proof = w / XCDS;
    } else {
        p.tile = id % tiles;
        p.proof = id / tiles;
    }
    p.valid = p.tile < tiles && p.proof < batch;
    return p;
}

}  // namespace qmap
