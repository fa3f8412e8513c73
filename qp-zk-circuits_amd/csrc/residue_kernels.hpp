// residue_kernels.hpp — launchers of residue_kernels.hip: the needle scan over one buffer and a zero fill.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "../../include/qpgpu.h"

// the needles travel in the kernel arguments (uniform: scalar registers); unused slots are never compared
struct ResidueNeedles { uint64_t v[QPGPU_RESIDUE_MAX_NEEDLES]; uint32_t n; };
// the small result block of one launch: match count and the first RESIDUE_DEV_CAP matches, in no particular order
constexpr uint32_t RESIDUE_DEV_CAP = 64;
struct ResidueResult { unsigned long long count; struct { uint64_t word, offset_words; } found[RESIDUE_DEV_CAP]; };

// compares each of the `words` 64-bit words at buf (16-byte aligned) with every needle; res must be zeroed before the launch
hipError_t rk_scan(const uint64_t *buf, uint64_t words, const ResidueNeedles &needles, ResidueResult *res, hipStream_t st);
// zero fill by a kernel: for device memory and for pinned host memory alike (stream-ordered behind the last reader of either)
hipError_t rk_zero(void *dst, size_t bytes, hipStream_t st);
