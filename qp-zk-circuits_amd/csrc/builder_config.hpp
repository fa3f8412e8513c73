// builder_config.hpp — a caller's CircuitConfig (include/qpgpu_wire.h) carried over into the native builder's Config, for every
// circuit entry that takes one (leaf_circuit.cpp, wrapper_circuit.cpp): one policy, so that the leaf and the wrappers cannot drift.
#pragma once
#include <cstddef>
#include "../../include/qpgpu_wire.h"
#include "builder.hpp"

namespace cb {
// user = NULL: qpgpu_wormhole_circuit_config(level). The config goes through qpgpu_validate_circuit_config first (a refusal carries
// its message as it is); then what the builder does not model is refused by name behind "<entry>: ": security_bits other than
// standard_recursion_config's 100, use_base_arithmetic_gate = false, fields beyond 16 bits, proof_of_work_bits above 32,
// reduction arity bits outside 1..4, final polynomial bits above 8 (max_quotient_degree_factor other than 8 and num_constants other
// than 2 are Config::validate's, in the Builder's constructor). Returns QPGPU_OK or QPGPU_EINVAL with the reason in err.
int config_from_circuit_config(const char *entry, int level, const qpgpu_circuit_config *user, Config &cfg, char *err, size_t err_cap);
}  // namespace cb
