// builder_config.cpp — see builder_config.hpp. Host only.
#include "builder_config.hpp"
#include <cstdio>
#include "../../include/qpgpu.h"

namespace cb {

// WormholeProver::new(config) / WormholeCircuit::new(config) (wormhole/prover/src/lib.rs:137-149, circuit/src/circuit.rs:115-152) and the
// batch layers' PrivateBatchCircuit::new(config, ..) / PublicBatchCircuit::new(config, ..) (private_batch/circuit/circuit_logic.rs:88,
// public_batch/circuit/circuit_logic.rs:63): the caller's CircuitConfig, or the level's canonical one for NULL, checked the way every
// Wormhole circuit constructor checks it (validate_circuit_config, with its messages) and carried over into the builder's Config. The two
// fields the builder does not model must hold standard_recursion_config's values: a config that asks for anything else is refused, not
// built as something it is not.
int config_from_circuit_config(const char *entry, int level, const qpgpu_circuit_config *user, Config &cfg, char *err, size_t err_cap) {
    auto fail = [&](const std::string &m) { if (err) std::snprintf(err, err_cap, "%s", m.c_str()); return QPGPU_EINVAL; };
    const std::string pre = std::string(entry) + ": circuit config ";
    qpgpu_circuit_config std_cfg;
    if (qpgpu_wormhole_circuit_config(level, &std_cfg) != 0) return fail(std::string(entry) + ": unknown circuit level");
    const qpgpu_circuit_config c = user ? *user : std_cfg;
    char why[QPGPU_CONFIG_ERR_CAP];
    why[0] = 0;
    if (qpgpu_validate_circuit_config(&c, why) != 0) return fail(why);
    if (c.security_bits != std_cfg.security_bits)
        return fail(pre + "security_bits (" + std::to_string(c.security_bits) + ") is not modelled by this builder; only " +
                    std::to_string(std_cfg.security_bits) + " (standard_recursion_config) is accepted");
    if ((c.use_base_arithmetic_gate != 0) != (std_cfg.use_base_arithmetic_gate != 0))
        return fail(pre + "use_base_arithmetic_gate = false is not modelled by this builder; only true (standard_recursion_config) is accepted");
    const struct { const char *name; uint64_t v; unsigned *to; } f[11] = {
        {"num_wires", c.num_wires, &cfg.num_wires}, {"num_routed_wires", c.num_routed_wires, &cfg.num_routed_wires}, {"num_constants", c.num_constants, &cfg.num_constants},
        {"num_challenges", c.num_challenges, &cfg.num_challenges}, {"max_quotient_degree_factor", c.max_quotient_degree_factor, &cfg.max_quotient_degree_factor},
        {"fri_config.rate_bits", c.rate_bits, &cfg.rate_bits}, {"fri_config.cap_height", c.cap_height, &cfg.cap_height},
        {"fri_config.proof_of_work_bits", c.proof_of_work_bits, &cfg.proof_of_work_bits}, {"fri_config.num_query_rounds", c.num_query_rounds, &cfg.num_query_rounds},
        {"fri_config.reduction_strategy arity_bits", c.reduction_arity_bits, &cfg.arity_bits}, {"fri_config.reduction_strategy final_poly_bits", c.reduction_final_poly_bits, &cfg.final_poly_bits}};
    for (const auto &x : f) {
        if (x.v > 0xFFFFu) return fail(pre + x.name + " (" + std::to_string(x.v) + ") out of range");
        *x.to = (unsigned)x.v;
    }
    // what the prover's transcript and FRI code take for granted about these three (Builder::validate covers the rest)
    if (cfg.proof_of_work_bits > 32) return fail(pre + "fri_config.proof_of_work_bits (" + std::to_string(c.proof_of_work_bits) + ") must be <= 32");
    if (cfg.arity_bits == 0 || cfg.arity_bits > 4) return fail(pre + "fri_config.reduction_strategy arity_bits (" + std::to_string(c.reduction_arity_bits) + ") must be 1..4");
    if (cfg.final_poly_bits > 8) return fail(pre + "fri_config.reduction_strategy final_poly_bits (" + std::to_string(c.reduction_final_poly_bits) + ") must be <= 8");
    cfg.zero_knowledge = c.zero_knowledge != 0;
    return QPGPU_OK;
}

}  // namespace cb
