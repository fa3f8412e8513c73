// explain_kernels.hpp — launchers of explain_kernels.hip: the kernels qpgpu_circuit_explain_witness (explain_api.cpp) adds around
// the gate kernels of the witness check. None of them evaluates a gate: they mark, move and compare values.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

// bitmap bit i (word i / 32, bit i % 32; the caller has zeroed it) = row i has a non-zero sum in one of the nch columns of
// acc ([nch][n], the gate sums of the trace rows as pk_gate_sums leaves them)
hipError_t ek_failing_rows(const uint64_t *acc, uint64_t n, uint32_t nch, uint32_t *bitmap, hipStream_t st);
// compact trace of the rows rows[0..count): dst[col * stride + k] = src[col * n + rows[k]] for k < count, 0 for count <= k < stride
// (stride >= count). One call per matrix: the wires, then the selector and constant columns.
hipError_t ek_gather_rows(const uint64_t *src, uint64_t n, uint32_t cols, const uint32_t *rows, uint32_t count, uint32_t stride, uint64_t *dst, hipStream_t st);
// the weight table of one expansion pass, [nch][nterms]: zero everywhere but a 1 at [c][t0 + k0 + c] for every column c with
// k0 + c < num_constraints, i.e. column c is the indicator of constraint k0 + c of the gates
hipError_t ek_one_hot(uint64_t *table, uint32_t nch, uint32_t nterms, uint32_t t0, uint32_t k0, uint32_t num_constraints, hipStream_t st);
// bitmap bit (row * num_routed + wire) = that routed cell's value differs (canonically) from the value at src_of[row * num_routed +
// wire] (a flat cell, column * n + row); the caller has zeroed the bitmap
hipError_t ek_copy_mismatches(const uint64_t *wires, const uint32_t *src_of, uint64_t n, uint32_t num_routed, uint32_t *bitmap, hipStream_t st);
// for the cells cells[0..count) (row * num_routed + wire): out[3 i] = the cell's value, out[3 i + 1] = the value at its class's
// source, out[3 i + 2] = that source (flat, column * n + row); values canonical
hipError_t ek_fetch_cells(const uint64_t *wires, const uint32_t *src_of, uint64_t n, uint32_t num_routed, const uint64_t *cells, uint32_t count, uint64_t *out, hipStream_t st);
