"""ctypes binding of include/qpgpu.h. Thin: argument marshalling and error mapping only."""
import ctypes
import dataclasses
import os

import numpy as np

P = 0xFFFFFFFF00000001
MULT_GEN = 14293326489335486720

NTT_FORWARD = 0
NTT_INVERSE = 1
NTT_OUT_BITREV = 2

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path():
    return os.path.join(_HERE, "libqpgpu.so")


class QpGpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"qpgpu error {code}: {msg}")
        self.code = code


_lib = None


def load_library():
    """Load libqpgpu.so. Raises if it has not been built (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = ctypes.CDLL(path)
    c = ctypes
    vp, u64p = c.c_void_p, c.c_void_p
    sigs = {
        "qpgpu_version": (c.c_char_p, []),
        "qpgpu_ctx_pci_bus_id": (c.c_int, [c.c_void_p, c.c_char_p, c.c_size_t]),
        "qpgpu_verifier_create": (c.c_int, [vp, c.c_size_t, vp, c.c_size_t, c.c_int, vp, c.c_size_t, c.POINTER(vp), c.c_char_p]),
        "qpgpu_verifier_free": (None, [vp]),
        "qpgpu_verifier_proof_size": (c.c_size_t, [vp]),
        "qpgpu_verifier_constants_sigmas_cap": (c.c_int, [vp, vp, c.c_size_t]),
        "qpgpu_verifier_verify": (c.c_int, [vp, c.c_char_p, c.c_size_t, c.c_char_p]),
        "qpgpu_verifier_verify_many": (c.c_int, [vp, vp, vp, c.c_size_t, c.c_uint, vp, c.c_char_p]),
        "qpgpu_verifier_verify_many_device": (c.c_int, [vp, vp, vp, vp, c.c_size_t, c.c_uint, vp, vp, c.c_char_p]),
        "qpgpu_verifier_verify_many_device_ex": (c.c_int, [vp, vp, vp, vp, c.c_size_t, c.c_uint, c.c_uint, vp, vp, c.c_char_p]),
        "qpgpu_fri_verifier_create": (c.c_int, [vp, c.c_int, vp, c.c_size_t, c.POINTER(vp), c.c_char_p]),
        "qpgpu_fri_verifier_free": (None, [vp]),
        "qpgpu_fri_verifier_proof_size": (c.c_size_t, [vp]),
        "qpgpu_fri_verifier_num_openings": (c.c_size_t, [vp]),
        "qpgpu_fri_verifier_challenges": (c.c_int, [vp, vp, c.c_char_p, c.c_size_t, u64p, u64p, c.POINTER(c.c_uint64), u64p, c.c_char_p]),
        "qpgpu_fri_verify": (c.c_int, [vp, vp, u64p, u64p, u64p, u64p, c.c_uint64, u64p, c.c_char_p, c.c_size_t, c.c_char_p]),
        "qpgpu_fri_verify_many_device": (c.c_int, [vp, vp, c.c_size_t, vp, vp, u64p, u64p, u64p, u64p, u64p, u64p, vp, vp, vp, vp, c.c_char_p]),
        "qpgpu_ctx_create": (c.c_int, [c.c_int, c.POINTER(vp)]),
        "qpgpu_ctx_destroy": (None, [vp]),
        "qpgpu_last_error": (c.c_char_p, [vp]),
        "qpgpu_ctx_set_stream": (c.c_int, [vp, vp]),
        "qpgpu_sync": (c.c_int, [vp]),
        "qpgpu_profile_enable": (c.c_int, [vp, c.c_int]),
        "qpgpu_profile_read": (c.c_int, [vp, c.c_char_p, c.POINTER(c.c_double), c.POINTER(c.c_uint64)]),
        "qpgpu_malloc": (c.c_int, [vp, c.c_size_t, c.POINTER(vp)]),
        "qpgpu_free": (c.c_int, [vp, vp]),
        "qpgpu_free_scrubbed": (c.c_int, [vp, vp, c.c_size_t]),
        "qpgpu_memcpy_h2d": (c.c_int, [vp, vp, vp, c.c_size_t]),
        "qpgpu_memcpy_d2h": (c.c_int, [vp, vp, vp, c.c_size_t]),
        "qpgpu_memcpy_d2d": (c.c_int, [vp, vp, vp, c.c_size_t]),
        "qpgpu_ntt_batch": (c.c_int, [vp, u64p, c.c_uint, c.c_size_t, c.c_int, c.c_uint64]),
        "qpgpu_ntt_batch_dev": (c.c_int, [vp, u64p, u64p, c.c_uint, c.c_size_t, c.c_int, c.c_uint64]),
        "qpgpu_lde_batch_dev": (c.c_int, [vp, u64p, u64p, c.c_uint, c.c_uint, c.c_size_t, c.c_int, c.c_uint64]),
        "qpgpu_poseidon_permute_dev": (c.c_int, [vp, u64p, c.c_size_t]),
        "qpgpu_poseidon2_hash_pad10_dev": (c.c_int, [vp, u64p, c.c_size_t, u64p, c.c_size_t, c.c_size_t, u64p]),
        "qpgpu_poseidon2_qp_params": (c.c_size_t, [u64p, c.c_size_t]),
        # the chain's 4-ary ZK Merkle tree on the device (include/qpgpu_leaf.h; wrapped by leaf.ZkTree)
        "qpgpu_zk_leaf_hash_batch": (c.c_int, [vp, vp, c.c_size_t, vp]),
        "qpgpu_zk_tree_build": (c.c_int, [vp, vp, c.c_size_t, c.c_uint, c.c_uint, c.POINTER(vp), c.c_char_p]),
        "qpgpu_zk_tree_free": (None, [vp]),
        "qpgpu_zk_tree_depth": (c.c_uint, [vp]),
        "qpgpu_zk_tree_leaf_count": (c.c_size_t, [vp]),
        "qpgpu_zk_tree_root": (c.c_int, [vp, vp]),
        "qpgpu_zk_tree_read_level": (c.c_int, [vp, c.c_uint, c.c_size_t, c.c_size_t, vp]),
        "qpgpu_zk_tree_open": (c.c_int, [vp, vp, c.c_size_t, vp, vp]),
        "qpgpu_zk_tree_build_reserved": (c.c_int, [vp, vp, c.c_size_t, c.c_size_t, c.c_uint, c.c_uint, c.POINTER(vp), c.c_char_p]),
        "qpgpu_zk_tree_capacity": (c.c_size_t, [vp]),
        "qpgpu_zk_tree_append": (c.c_int, [vp, vp, c.c_size_t, c.c_uint, vp, c.c_char_p]),
        "qpgpu_zk_tree_snapshot": (c.c_int, [vp, vp]),
        "qpgpu_zk_tree_open_at": (c.c_int, [vp, vp, vp, c.c_size_t, vp, vp]),
        "qpgpu_zk_tree_snapshots_at": (c.c_int, [vp, vp, c.c_size_t, vp]),
        "qpgpu_zk_tree_snapshot_check": (c.c_int, [vp, vp]),
        "qpgpu_zk_tree_open_at_counts": (c.c_int, [vp, vp, vp, c.c_size_t, vp, vp, vp]),
        "qpgpu_zk_tree_truncate": (c.c_int, [vp, c.c_size_t, vp, c.c_char_p]),
        "qpgpu_poseidon2_hash_pad10": (c.c_int, [u64p, c.c_size_t, u64p, c.c_size_t, u64p]),
        "qpgpu_crash_trace_armed": (c.c_int, []),
        "qpgpu_circuit_num_public_inputs": (c.c_size_t, [vp]),
        "qpgpu_merkle_digest_count": (c.c_size_t, [c.c_uint, c.c_uint]),
        "qpgpu_merkle_build_dev": (c.c_int, [vp, u64p, c.c_uint64, c.c_uint32, c.c_uint, c.c_uint, u64p, u64p]),
        "qpgpu_merkle_build_rows_dev": (c.c_int, [vp, u64p, c.c_uint32, c.c_uint, c.c_uint, u64p, u64p]),
        "qpgpu_circuit_load": (c.c_int, [vp, u64p, c.c_size_t, c.POINTER(vp)]),
        "qpgpu_circuit_load_batch": (c.c_int, [vp, u64p, c.c_size_t, c.c_uint, c.POINTER(vp)]),
        "qpgpu_circuit_max_batch": (c.c_uint, [vp]),
        "qpgpu_circuit_scrub": (c.c_int, [vp]),
        "qpgpu_prove_batch_dev": (c.c_int, [vp, vp, c.c_uint32, vp, vp, c.c_size_t, vp]),
        "qpgpu_ctx_set_hasher": (c.c_int, [vp, c.c_int, u64p, c.c_size_t]),
        "qpgpu_ctx_get_hasher": (c.c_int, [vp]),
        "qpgpu_ctx_challenger_observe": (c.c_int, [vp, vp, u64p, c.c_size_t]),
        "qpgpu_ctx_challenger_get": (c.c_int, [vp, vp, c.POINTER(c.c_uint64)]),
        "qpgpu_pool_create_batched": (c.c_int, [c.c_int, u64p, c.c_size_t, c.c_uint, c.c_uint, c.POINTER(vp)]),
        "qpgpu_circuit_free": (None, [vp]),
        "qpgpu_circuit_constants_sigmas_cap": (c.c_int, [vp, u64p, c.c_size_t]),
        "qpgpu_proof_size": (c.c_size_t, [vp]),
        "qpgpu_circuit_set_blinding_seed": (c.c_int, [vp, c.c_uint64]),
        "qpgpu_circuit_set_witness_check": (c.c_int, [vp, c.c_int]),
        "qpgpu_circuit_explain_witness": (c.c_int, [vp, u64p, c.c_int, u64p, c.c_uint32, c.c_uint, vp, c.c_size_t, c.POINTER(c.c_size_t),
                                                    c.POINTER(c.c_uint64), c.POINTER(c.c_uint64)]),
        "qpgpu_witness_finding_format": (c.c_int, [u64p, c.c_size_t, vp, c.c_char_p, c.c_size_t]),
        "qpgpu_circuit_set_quotient_fused": (c.c_int, [vp, c.c_int]),
        "qpgpu_circuit_quotient_info": (c.c_int, [vp, c.POINTER(c.c_int), c.POINTER(c.c_int)]),
        "qpgpu_circuit_quotient_pair_info": (c.c_int, [vp, c.POINTER(c.c_int), c.POINTER(c.c_int)]),
        "qpgpu_circuit_gate_rows": (c.c_int, [vp, c.c_uint, vp, c.c_size_t, c.POINTER(c.c_size_t)]),
        "qpgpu_prove": (c.c_int, [vp, u64p, u64p, vp, c.c_size_t, c.POINTER(c.c_size_t)]),
        "qpgpu_prove_dev": (c.c_int, [vp, u64p, u64p, vp, c.c_size_t, c.POINTER(c.c_size_t)]),
        "qpgpu_poseidon_constants": (c.c_size_t, [u64p, u64p, c.c_size_t]),
        "qpgpu_pool_create": (c.c_int, [c.c_int, u64p, c.c_size_t, c.c_uint, c.POINTER(vp)]),
        "qpgpu_pool_destroy": (None, [vp]),
        "qpgpu_pool_proof_size": (c.c_size_t, [vp]),
        "qpgpu_pool_workers": (c.c_uint, [vp]),
        "qpgpu_pool_last_error": (c.c_char_p, [vp]),
        "qpgpu_pool_submit": (c.c_int, [vp, u64p, u64p, vp, c.c_size_t, c.POINTER(c.c_uint64)]),
        "qpgpu_pool_wait": (c.c_int, [vp, c.c_uint64, c.POINTER(c.c_size_t)]),
        "qpgpu_pool_set_witness_check": (c.c_int, [vp, c.c_int]),
        "qpgpu_pool_create_multi": (c.c_int, [vp, c.c_uint, u64p, c.c_size_t, c.c_uint, c.c_uint, c.c_uint, c.POINTER(vp)]),
        "qpgpu_pool_devices": (c.c_uint, [vp]),
        "qpgpu_pool_serialized": (c.c_int, [vp]),
        "qpgpu_pool_set_partial_cells": (c.c_int, [vp, u64p, c.c_size_t]),
        "qpgpu_pool_set_partial_cells_blinded": (c.c_int, [vp, u64p, c.c_size_t, c.c_size_t]),
        "qpgpu_pool_submit_on": (c.c_int, [vp, c.c_uint, u64p, u64p, vp, c.c_size_t, c.POINTER(c.c_uint64)]),
        "qpgpu_pool_submit_host": (c.c_int, [vp, u64p, u64p, vp, c.c_size_t, c.POINTER(c.c_uint64)]),
        "qpgpu_pool_submit_partial": (c.c_int, [vp, u64p, u64p, vp, c.c_size_t, c.POINTER(c.c_uint64)]),
        "qpgpu_set_hasher": (c.c_int, [c.c_int, u64p, c.c_size_t]),
        "qpgpu_get_hasher": (c.c_int, []),
        "qpgpu_witness_info": (c.c_int, [vp, c.POINTER(c.c_uint64), c.POINTER(c.c_uint64), c.POINTER(c.c_uint64)]),
        "qpgpu_witness_free_mask": (c.c_int, [vp, vp, c.c_size_t]),
        "qpgpu_generate_witness_dev": (c.c_int, [vp, u64p, u64p]),
        "qpgpu_generate_witness": (c.c_int, [vp, u64p, u64p]),
        "qpgpu_generate_witness_batch_dev": (c.c_int, [vp, u64p, c.c_uint32, u64p]),
        "qpgpu_generate_witness_partial_dev": (c.c_int, [vp, u64p, u64p, c.c_size_t, u64p, u64p]),
        "qpgpu_generate_witness_partial_batch_dev": (c.c_int, [vp, u64p, c.c_size_t, u64p, u64p, c.c_uint32, u64p, vp]),
        "qpgpu_generate_witness_partial_batch_blinded_dev": (c.c_int, [vp, u64p, c.c_size_t, c.c_size_t, u64p, c.c_char_p, u64p, c.c_uint32, u64p, vp]),
        "qpgpu_witness_public_inputs_dev": (c.c_int, [vp, u64p, c.c_uint32, u64p]),
        "qpgpu_witness_partial_prepare": (c.c_int, [vp, u64p, c.c_size_t, c.c_uint32]),
        "qpgpu_oracle_commit": (c.c_int, [vp, u64p, c.c_uint32, c.c_uint, c.c_uint, c.c_uint, c.c_uint, c.c_uint64, c.c_uint32,
                                          c.POINTER(vp)]),
        "qpgpu_oracle_free": (None, [vp]),
        "qpgpu_oracle_cap": (c.c_int, [vp, u64p, c.c_size_t]),
        "qpgpu_oracle_eval": (c.c_int, [vp, u64p, c.c_uint32, c.c_uint32, u64p]),
        "qpgpu_oracle_read": (c.c_int, [vp, c.c_uint, c.c_uint32, c.c_uint32, u64p]),
        "qpgpu_oracle_device_ptrs": (c.c_int, [vp, c.POINTER(vp), c.POINTER(vp), c.POINTER(vp)]),
        "qpgpu_oracle_open": (c.c_int, [vp, u64p, c.c_size_t, u64p, u64p]),
        "qpgpu_oracle_leaf_width": (c.c_size_t, [vp]),
        "qpgpu_oracle_commit_sharded": (c.c_int, [c.POINTER(vp), c.c_uint32, u64p, c.c_uint32, c.c_uint, c.c_uint, c.c_uint, c.c_uint,
                                                  c.c_uint64, c.c_uint32, c.POINTER(vp)]),
        "qpgpu_oracle_shards": (c.c_uint32, [vp]),
        "qpgpu_oracle_shard_range": (c.c_int, [vp, c.c_uint32, c.POINTER(c.c_uint64), c.POINTER(c.c_uint64)]),
        "qpgpu_oracle_shard_device_ptrs": (c.c_int, [vp, c.c_uint32, c.POINTER(vp), c.POINTER(vp)]),
        "qpgpu_stage_plan_create": (c.c_int, [vp, u64p, c.c_size_t, vp, c.POINTER(vp), c.c_char_p]),
        "qpgpu_stage_plan_create_sharded": (c.c_int, [vp, u64p, c.c_size_t, vp, c.POINTER(vp), c.c_char_p]),
        "qpgpu_stage_plan_shards": (c.c_uint32, [vp]),
        "qpgpu_stage_plan_free": (None, [vp]),
        "qpgpu_stage_plan_info": (c.c_int, [vp, c.POINTER(c.c_uint), c.POINTER(c.c_uint), c.POINTER(c.c_uint), c.POINTER(c.c_uint),
                                            c.POINTER(c.c_int)]),
        "qpgpu_stage_partial_products": (c.c_int, [vp, u64p, c.c_int, u64p, u64p, u64p]),
        "qpgpu_stage_quotient": (c.c_int, [vp, vp, vp, u64p, u64p, u64p, u64p, u64p]),
        "qpgpu_challenger_init": (None, [vp]),
        "qpgpu_challenger_observe": (None, [vp, u64p, c.c_size_t]),
        "qpgpu_challenger_get": (c.c_uint64, [vp]),
        "qpgpu_fri_proof_size": (c.c_size_t, [c.POINTER(vp), c.c_uint32, vp]),
        "qpgpu_fri_prove": (c.c_int, [vp, c.POINTER(vp), c.c_uint32, vp, c.c_uint32, vp, vp, vp, c.c_size_t,
                                      c.POINTER(c.c_size_t)]),
        "qpgpu_fri_begin": (c.c_int, [vp, c.POINTER(vp), c.c_uint32, vp, c.c_uint32, vp, u64p, c.POINTER(vp)]),
        "qpgpu_fri_round_commit": (c.c_int, [vp, u64p, c.c_size_t]),
        "qpgpu_fri_round_fold": (c.c_int, [vp, u64p]),
        "qpgpu_fri_final_poly": (c.c_int, [vp, u64p, c.c_size_t, c.POINTER(c.c_size_t)]),
        "qpgpu_fri_query_size": (c.c_size_t, [vp]),
        "qpgpu_fri_open": (c.c_int, [vp, u64p, c.c_size_t, vp, c.c_size_t, c.POINTER(c.c_size_t)]),
        "qpgpu_fri_session_free": (None, [vp]),
        "qpgpu_fri_grind": (c.c_int, [vp, vp, c.c_uint, c.POINTER(c.c_uint64)]),
        # lockstep batches of the stage flow
        "qpgpu_oracle_commit_batch": (c.c_int, [vp, c.POINTER(vp), c.c_uint32, c.c_uint32, c.c_uint, c.c_uint, c.c_uint, c.c_uint,
                                                c.c_uint64, c.c_uint32, c.POINTER(vp)]),
        "qpgpu_oracle_batch": (c.c_uint32, [vp]),
        "qpgpu_oracle_strides": (c.c_int, [vp, c.POINTER(c.c_uint64), c.POINTER(c.c_uint64), c.POINTER(c.c_uint64)]),
        "qpgpu_oracle_eval_batch": (c.c_int, [vp, u64p, c.c_uint32, c.c_uint32, u64p]),
        "qpgpu_oracle_open_batch": (c.c_int, [vp, u64p, c.c_size_t, u64p, u64p]),
        "qpgpu_stage_plan_create_batch": (c.c_int, [vp, u64p, c.c_size_t, vp, c.c_uint32, c.POINTER(vp), c.c_char_p]),
        "qpgpu_stage_plan_max_batch": (c.c_uint32, [vp]),
        "qpgpu_stage_partial_products_batch": (c.c_int, [vp, c.POINTER(vp), c.c_uint32, c.c_int, u64p, u64p, u64p]),
        "qpgpu_stage_quotient_batch": (c.c_int, [vp, vp, vp, c.c_uint32, u64p, u64p, u64p, u64p, u64p]),
        "qpgpu_fri_prove_batch": (c.c_int, [vp, c.POINTER(vp), c.c_uint32, vp, c.c_uint32, u64p, c.c_uint32, vp, vp, c.POINTER(vp),
                                            c.c_size_t, c.POINTER(c.c_size_t)]),
        "qpgpu_fri_begin_batch": (c.c_int, [vp, c.POINTER(vp), c.c_uint32, vp, c.c_uint32, u64p, c.c_uint32, vp, u64p, c.POINTER(vp)]),
        "qpgpu_fri_session_batch": (c.c_uint32, [vp]),
        "qpgpu_fri_grind_batch": (c.c_int, [vp, vp, c.c_uint32, c.c_uint, c.POINTER(c.c_uint64)]),
        "qpgpu_field_probe": (c.c_int, [vp, c.c_uint, c.c_uint, u64p, u64p, c.c_size_t, u64p, c.c_size_t, c.c_int]),
        "qpgpu_synth_pack_words": (c.c_size_t, [c.c_uint, c.c_uint, c.c_uint]),
        "qpgpu_synth_pack_words_ex": (c.c_size_t, [c.c_uint, c.c_uint, c.c_uint, c.c_uint]),
        "qpgpu_synth_p2_sites": (c.c_size_t, [c.c_uint, c.c_uint, c.c_uint, u64p, c.c_size_t]),
        "qpgpu_synth_circuit_ex": (c.c_int, [c.c_uint, c.c_uint, c.c_uint, c.c_uint, c.c_uint64, c.c_uint, u64p, c.c_size_t,
                                             c.POINTER(c.c_size_t), u64p, u64p]),
        "qpgpu_synth_circuit": (c.c_int, [c.c_uint, c.c_uint, c.c_uint, c.c_uint, c.c_uint64, u64p, c.c_size_t,
                                          c.POINTER(c.c_size_t), u64p, u64p]),
        "qpgpu_ctx_residue_scan": (c.c_int, [vp, u64p, c.c_size_t, c.c_uint64, c.POINTER(c.c_uint64), vp, c.c_size_t, c.POINTER(c.c_uint64)]),
        "qpgpu_residue_region_name": (c.c_char_p, [c.c_uint32]),
        "qpgpu_ctx_residue_audit_begin": (c.c_int, [vp, u64p, c.c_size_t]),
        "qpgpu_ctx_residue_audit_end": (c.c_int, [vp, c.POINTER(c.c_uint64), vp, c.c_size_t, c.POINTER(c.c_uint64)]),
        "qpgpu_pool_scrub": (c.c_int, [vp]),
        "qpgpu_pool_residue_scan": (c.c_int, [vp, u64p, c.c_size_t, c.c_uint64, c.POINTER(c.c_uint64), vp, c.c_size_t, c.POINTER(c.c_uint64)]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def exported_symbols():
    """Names include/qpgpu.h declares; tests check each resolves in the built library."""
    import glob
    import re
    names = set()
    for hdr in glob.glob(os.path.join(os.path.dirname(_HERE), "include", "*.h")):
        names |= set(re.findall(r"\b(qpgpu_[a-z0-9_]+)\s*\(", open(hdr).read()))
    return sorted(names)


def set_hasher_poseidon():
    """Process default (what NEW contexts and the context-free helpers use): plonky2's Poseidon."""
    load_library().qpgpu_set_hasher(0, None, 0)


def _p2_block(rc_ext, rc_int, diag_m1, m4):
    return np.concatenate([np.asarray(rc_ext, dtype=np.uint64).ravel(), np.asarray(rc_int, dtype=np.uint64).ravel(),
                           np.asarray(diag_m1, dtype=np.uint64).ravel(), np.asarray(m4, dtype=np.uint64).ravel()])


def set_hasher_poseidon2(rc_ext, rc_int, diag_m1, m4):
    """Process default: Poseidon2 with the given parameters (external round constants [8][12], internal [22], diagonal
    [12], 4x4 block). Contexts that already exist keep their hasher; QpGpu(hasher=...) sets one context's."""
    flat = _p2_block(rc_ext, rc_int, diag_m1, m4)
    rc = load_library().qpgpu_set_hasher(1, flat.ctypes.data, flat.size)
    if rc != 0:
        raise QpGpuError(rc, "qpgpu_set_hasher: bad Poseidon2 parameter block")


def poseidon2_qp_params():
    """qp-poseidon-core 3.1.0's Poseidon2 parameter set as the library carries it (pinned by the reference's seven known-answer
    vectors): (rc_ext[8,12], rc_int[22], diag_m1[12], m4[4,4]) — the arguments of set_hasher_poseidon2 / QpGpu(hasher=...)."""
    flat = np.empty(146, dtype=np.uint64)
    n = load_library().qpgpu_poseidon2_qp_params(flat.ctypes.data, flat.size)
    assert n == 146
    return flat[:96].reshape(8, 12).copy(), flat[96:118].copy(), flat[118:130].copy(), flat[130:146].reshape(4, 4).copy()


def poseidon_constants():
    """(round_constants[360], fast_partial[flat]) as derived by the library at start-up. Host only."""
    lib = load_library()
    n = lib.qpgpu_poseidon_constants(None, None, 0)
    rc = np.empty(360, dtype=np.uint64); fp = np.empty(n, dtype=np.uint64)
    lib.qpgpu_poseidon_constants(rc.ctypes.data, fp.ctypes.data, n)
    return rc, fp


# ---- test hook: the field probe (include/qpgpu.h, QPGPU_FP_*) ----
FP_OPS = ("canon", "add", "sub", "neg", "mul", "sqr", "reduce128", "reduce96", "mul_eps", "add_canonical", "mul7", "inv", "pow",
          "mul_pow2", "mul_pow2_dyn", "mul_group", "acc", "e2_add", "e2_sub", "e2_mul", "e2_scale", "e2_inv", "e2_pow", "dif_regs",
          "dif_sparse")
FP = {name: i for i, name in enumerate(FP_OPS)}


def field_probe_shape(op, param=0):
    """(words of a, words of b, words of out) per index, as the header's table has them."""
    name = FP_OPS[op]
    if name in ("mul_group", "acc"):
        return (param, param, param if name == "mul_group" else 1)
    if name in ("e2_add", "e2_sub", "e2_mul"):
        return (2, 2, 2)
    if name in ("e2_scale", "e2_pow"):
        return (2, 1, 2)
    if name == "e2_inv":
        return (2, 0, 2)
    if name in ("dif_regs", "dif_sparse"):
        return (1 << (param & 0xFF), 0, 1 << (param & 0xFF))
    return (1, 1 if name in ("add", "sub", "mul", "reduce128", "reduce96", "add_canonical", "pow") else 0, 1)


def _field_probe(ctx, op, a, b, param, on_device):
    op = FP[op] if isinstance(op, str) else int(op)
    wa, wb, wo = field_probe_shape(op, param)
    a = np.ascontiguousarray(a, dtype=np.uint64).ravel()
    b = np.ascontiguousarray(b, dtype=np.uint64).ravel() if b is not None else None
    n = a.size // wa if wa else 0
    if wa == 0 or a.size != n * wa or (wb and (b is None or b.size != n * wb)):
        raise ValueError("field_probe: operand lengths do not match the operation's words per index")
    out = np.empty(n * wo, dtype=np.uint64)
    rc = load_library().qpgpu_field_probe(ctx, op, param, a.ctypes.data, b.ctypes.data if b is not None else None, n,
                                          out.ctypes.data, out.size, 1 if on_device else 0)
    return rc, out


def field_probe_host(op, a, b=None, param=0):
    """qpgpu_field_probe through the host versions of the field primitives: no context, no GPU. op: a name of FP_OPS or its
    number. Returns the raw result words (flat)."""
    rc, out = _field_probe(None, op, a, b, param, False)
    if rc != 0:
        raise QpGpuError(rc, "qpgpu_field_probe: bad argument or an operation the host path does not have")
    return out


def synth_flags(poseidon=False, base_sum=False, ext_arith=False, recursion=False, hints=False, poseidon2=False, p2_alt_layout=False):
    return ((1 if poseidon else 0) | (2 if base_sum else 0) | (4 if ext_arith else 0) | (8 if recursion else 0) | (16 if hints else 0) |
            (64 if poseidon2 else 0) | (128 if p2_alt_layout else 0))


def synth_p2_sites(degree_bits, num_public_inputs=21, **kw):
    """Hash sites of a poseidon2=True synthetic circuit: list of (preimage length, gate rows, first slot); see include/qpgpu.h."""
    out = np.zeros(3 * 64, dtype=np.uint64)
    n = load_library().qpgpu_synth_p2_sites(degree_bits, num_public_inputs, synth_flags(**kw), out.ctypes.data, out.size)
    return [tuple(int(x) for x in out[3 * i:3 * i + 3]) for i in range(n)]


def synth_circuit(degree_bits, num_wires=135, num_routed=80, num_public_inputs=21, seed=1, poseidon=False, base_sum=False,
                  ext_arith=False, recursion=False, hints=False, poseidon2=False, p2_alt_layout=False):
    """Synthetic satisfied circuit: returns (pack_words, wires[num_wires, n], public_inputs). Host only.
    poseidon=True adds PoseidonGate rows (needs 135 wires), base_sum=True BaseSumGate<2> rows, ext_arith=True
    ArithmeticExtensionGate and MulExtensionGate rows, recursion=True Reducing / ReducingExtension / RandomAccess /
    Exponentiation / PoseidonMds rows, hints=True free-standing witness generators (a hint trailer in the pack)."""
    lib = load_library()
    flags = synth_flags(poseidon, base_sum, ext_arith, recursion, hints, poseidon2, p2_alt_layout)
    # with Poseidon rows the pack also carries the public-input cell trailer (2 + num_public_inputs words, circuit.hpp)
    words = lib.qpgpu_synth_pack_words_ex(degree_bits, num_wires, num_routed, flags) + 2 + num_public_inputs
    pack = np.empty(words, dtype=np.uint64)
    wires = np.empty((num_wires, 1 << degree_bits), dtype=np.uint64)
    pis = np.empty(num_public_inputs, dtype=np.uint64)
    got = ctypes.c_size_t()
    rc = lib.qpgpu_synth_circuit_ex(degree_bits, num_wires, num_routed, num_public_inputs, seed, flags, pack.ctypes.data,
                                    words, ctypes.byref(got), wires.ctypes.data, pis.ctypes.data)
    if rc != 0 or got.value > words:
        raise QpGpuError(rc, f"synth_circuit failed (words {got.value} vs {words})")
    return pack[:got.value].copy() if got.value != words else pack, wires, pis


class CircuitConfig(ctypes.Structure):
    """qpgpu_circuit_config (include/qpgpu_wire.h): plonky2's CircuitConfig with its FriConfig as plain data."""
    _fields_ = [(k, ctypes.c_uint64) for k in ("num_wires", "num_routed_wires", "num_constants", "security_bits", "num_challenges", "max_quotient_degree_factor")] + \
               [("use_base_arithmetic_gate", ctypes.c_int), ("zero_knowledge", ctypes.c_int)] + \
               [(k, ctypes.c_uint64) for k in ("rate_bits", "cap_height", "proof_of_work_bits", "num_query_rounds", "reduction_arity_bits", "reduction_final_poly_bits")]

    def replace(self, **fields):
        """A copy with the named fields changed."""
        other = CircuitConfig.from_buffer_copy(self)
        for k, v in fields.items():
            if k not in dict(self._fields_):
                raise TypeError("CircuitConfig has no field %r" % k)
            setattr(other, k, v)
        return other

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


CONFIG_LEVELS = {"leaf": 0, "private_batch": 1, "public_batch": 2}
CONFIG_ERR_CAP = 400


def circuit_config(level="leaf", **fields):
    """qpgpu_wormhole_circuit_config: the canonical config of a level ("leaf" / "public_batch": standard_recursion_config;
    "private_batch": the zero-knowledge one, 60 routed wires), optionally with fields changed. Host only."""
    lib = load_library()
    lib.qpgpu_wormhole_circuit_config.argtypes = [ctypes.c_int, ctypes.c_void_p]
    c = CircuitConfig()
    if lib.qpgpu_wormhole_circuit_config(CONFIG_LEVELS[level] if isinstance(level, str) else level, ctypes.byref(c)) != 0:
        raise ValueError("unknown circuit config level %r" % (level,))
    return c.replace(**fields) if fields else c


def as_circuit_config(config):
    """None, a level name, a CircuitConfig, or any object / mapping with qpgpu_circuit_config's fields -> CircuitConfig or None."""
    if config is None or isinstance(config, CircuitConfig):
        return config
    if isinstance(config, str):
        if config not in CONFIG_LEVELS:
            raise ValueError("unknown circuit config %r (one of %s, or a qpgpu_circuit_config-shaped object)" % (config, ", ".join(sorted(CONFIG_LEVELS))))
        return circuit_config(config)
    get = config.__getitem__ if hasattr(config, "__getitem__") else lambda k: getattr(config, k)
    c = CircuitConfig()
    for k, _ in CircuitConfig._fields_:
        setattr(c, k, int(get(k)))
    return c


def validate_circuit_config(config):
    """qpgpu_validate_circuit_config: None when every Wormhole circuit constructor would take the config, else the reference's message."""
    lib = load_library()
    lib.qpgpu_validate_circuit_config.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    err = ctypes.create_string_buffer(CONFIG_ERR_CAP)
    return None if lib.qpgpu_validate_circuit_config(ctypes.byref(as_circuit_config(config)), err) == 0 else err.value.decode()


class AggConfigArgs(ctypes.Structure):
    """qpgpu_agg_config_args (include/qpgpu_wire.h): the reference's AggConfigArgs (wormhole/memprof/src/config.rs) — overrides on top of
    the production private-batch config, each with a presence bit."""
    KNOBS = ("rate_bits", "cap_height", "num_wires", "num_routed_wires", "max_quotient_degree_factor", "num_query_rounds", "security_bits", "num_challenges")
    HAS = dict(zk_mode=1, **{k: 2 << i for i, k in enumerate(KNOBS)})
    ZK_MODES = {"rowblinding": 0, "disabled": 1}
    _fields_ = [("present", ctypes.c_uint32), ("zk_mode", ctypes.c_int)] + [(k, ctypes.c_uint64) for k in KNOBS] + [("allow_weakening_security", ctypes.c_int)]


def agg_config_args(allow_weakening_security=False, **knobs):
    """AggConfigArgs from keyword overrides: zk_mode="rowblinding" / "disabled", the numeric knobs of AggConfigArgs.KNOBS; a knob
    left out (or None) is unset."""
    a = AggConfigArgs()
    a.allow_weakening_security = 1 if allow_weakening_security else 0
    for k, v in knobs.items():
        if k not in AggConfigArgs.HAS:
            raise TypeError("AggConfigArgs has no knob %r" % k)
        if v is None:
            continue
        a.present |= AggConfigArgs.HAS[k]
        setattr(a, k, AggConfigArgs.ZK_MODES[v] if k == "zk_mode" else int(v))
    return a


def agg_config_validate(args):
    """AggConfigArgs::validate: None, or the reference's message."""
    lib = load_library()
    lib.qpgpu_agg_config_validate.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    err = ctypes.create_string_buffer(CONFIG_ERR_CAP)
    return None if lib.qpgpu_agg_config_validate(ctypes.byref(args), err) == 0 else err.value.decode()


def agg_config_build(args):
    """AggConfigArgs::build: the production private-batch config with the overrides applied (rate_bits re-balances num_query_rounds)."""
    lib = load_library()
    lib.qpgpu_agg_config_build.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    c = CircuitConfig()
    if lib.qpgpu_agg_config_build(ctypes.byref(args), ctypes.byref(c)) != 0:
        raise ValueError("agg_config_build: bad argument")
    return c


def parse_agg_config_flags(argv):
    """The aggregation-config flags of the reference's memprof command line ("--zk-mode rowblinding --num-routed-wires 54 ..") ->
    (AggConfigArgs, the other flags as a dict). A --zk-mode this library has no circuit for ("polyfri": the fork's second
    zero-knowledge mode is un-vendored) raises ValueError naming it."""
    knobs, other, allow = {}, {}, False
    it = iter(argv)
    for flag in it:
        if not flag.startswith("--"):
            raise ValueError("unexpected argument %r" % flag)
        name = flag[2:].replace("-", "_")
        if name in ("allow_weakening_security", "skip_leaf_gen"):
            allow, other = (True, other) if name == "allow_weakening_security" else (allow, dict(other, skip_leaf_gen=True))
            continue
        value = next(it, None)
        if value is None:
            raise ValueError("%s needs a value" % flag)
        if name == "zk_mode":
            if value not in AggConfigArgs.ZK_MODES:
                raise ValueError("--zk-mode %s: not a mode this library builds (rowblinding, disabled); the fork's second zero-knowledge mode is un-vendored" % value)
            knobs[name] = value
        elif name in AggConfigArgs.KNOBS:
            knobs[name] = int(value)
        else:
            other[name] = value
    return agg_config_args(allow_weakening_security=allow, **knobs), other


def pack_header(pack_words):
    """The fixed header of a circuit pack (csrc/circuit.hpp) as a dict. Host only."""
    names = ["degree_bits", "num_wires", "num_routed_wires", "num_constants", "num_selectors", "num_challenges",
             "quotient_degree_factor", "num_partial_products", "num_public_inputs", "rate_bits", "cap_height",
             "proof_of_work_bits", "num_query_rounds", "zero_knowledge", "num_gate_constraints", "num_gates", "num_arity_rounds"]
    return {k: int(v) for k, v in zip(names, pack_words[1:18])}


def pack_public_input_cells(pack_words):
    """Cells (row * num_wires + wire) of the public inputs from the pack's "PUBI1" trailer, or None."""
    h = pack_header(pack_words)
    pos = 18 + h["num_arity_rounds"] + 8 * h["num_gates"] + h["num_routed_wires"] + 4
    pos += (h["num_selectors"] + h["num_constants"] + h["num_routed_wires"]) << h["degree_bits"]
    while pos + 2 <= len(pack_words):
        magic, cnt = int(pack_words[pos]), int(pack_words[pos + 1])
        if magic == 0x31544E4948:
            pos += 2 + 8 * cnt
        elif magic == 0x3149425550:
            return np.array(pack_words[pos + 2:pos + 2 + cnt], dtype=np.uint64)
        else:
            break
    return None


P2_LAYOUT_FIELDS = ("w_input", "w_output", "w_swap", "w_delta", "w_full0", "w_partial", "w_full1", "first_round_wires", "constraint_order", "end_wire")
P2_NO_SWAP = 0xFFFFFFFF


def pack_trailers(pack_words):
    """(magic, first word index, count) of every optional trailer of a circuit pack, in order."""
    h = pack_header(pack_words)
    pos = 18 + h["num_arity_rounds"] + 8 * h["num_gates"] + h["num_routed_wires"] + 4
    pos += (h["num_selectors"] + h["num_constants"] + h["num_routed_wires"]) << h["degree_bits"]
    out = []
    while pos + 2 <= len(pack_words):
        magic, cnt = int(pack_words[pos]), int(pack_words[pos + 1])
        per = {0x31544E4948: 8, 0x3149425550: 1, 0x314C473250: 1}.get(magic)
        if per is None:
            break
        out.append((magic, pos + 2, cnt))
        pos += 2 + per * cnt
    return out


def pack_p2_layout(pack_words):
    """Wire layout of the Poseidon2 gate from the pack's "P2GL1" trailer as a dict, or None when the pack has none (the
    library then assumes the default layout, csrc/circuit.hpp)."""
    for magic, at, cnt in pack_trailers(pack_words):
        if magic == 0x314C473250 and cnt == len(P2_LAYOUT_FIELDS):
            return {k: int(v) for k, v in zip(P2_LAYOUT_FIELDS, pack_words[at:at + cnt])}
    return None


def p2_site_cells(pack_words, site):
    """Cells of one Poseidon2 hash site of a synthetic circuit (synth_p2_sites): (preimage cells, digest cells), each a list of
    (wire, row), by the placement rule documented at qpgpu_synth_p2_sites in include/qpgpu.h."""
    lay = pack_p2_layout(pack_words) or dict(zip(P2_LAYOUT_FIELDS, (0, 12, 24, 25, 29, 65, 87, 0, 0, 135)))
    ln, blocks, slot = site
    pre = []
    for i in range(ln):
        k, j = divmod(i, 8)
        pre.append((lay["w_input"] + j, 8 * slot + 3) if k == 0 else (4 * j + 2, 8 * (slot + k - 1) + 4))
    last = 8 * (slot + blocks - 1) + 3
    return pre, [(lay["w_output"] + i, last) for i in range(4)]


class DeviceBuffer:
    """Device allocation owned through the C ABI (hipMalloc underneath)."""

    def __init__(self, gpu, nbytes):
        self.gpu, self.nbytes = gpu, nbytes
        p = ctypes.c_void_p()
        gpu._check(gpu.lib.qpgpu_malloc(gpu.ctx, nbytes, ctypes.byref(p)))
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.gpu._check(self.gpu.lib.qpgpu_memcpy_h2d(self.gpu.ctx, self.ptr, arr.ctypes.data, arr.nbytes))
        return self

    def download(self, count=None, dtype=np.uint64):
        n = self.nbytes // np.dtype(dtype).itemsize if count is None else count
        out = np.empty(n, dtype=dtype)
        self.gpu._check(self.gpu.lib.qpgpu_memcpy_d2h(self.gpu.ctx, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self, scrub=False):
        """scrub=True for buffers that held a witness: zeroed on the device before release."""
        if self.ptr:
            if scrub:
                self.gpu.lib.qpgpu_free_scrubbed(self.gpu.ctx, self.ptr, self.nbytes)
            else:
                self.gpu.lib.qpgpu_free(self.gpu.ctx, self.ptr)
            self.ptr = None


FINDING_GATE, FINDING_COPY = 1, 2


class _WitnessFinding(ctypes.Structure):
    """qpgpu_witness_finding of include/qpgpu.h (56 bytes)."""
    _fields_ = [("kind", ctypes.c_uint32), ("gate", ctypes.c_uint32), ("constraint", ctypes.c_uint32), ("wire", ctypes.c_uint32),
                ("wire_b", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("row", ctypes.c_uint64), ("row_b", ctypes.c_uint64),
                ("value", ctypes.c_uint64), ("value_b", ctypes.c_uint64)]


@dataclasses.dataclass(frozen=True)
class WitnessFinding:
    """One finding of Circuit.explain_witness. kind FINDING_GATE: constraint `constraint` of gate `gate` (index into the pack's gate
    list) is `value` (filter * constraint) on `row`. kind FINDING_COPY: the routed cell (row, wire) holds `value`, the source cell
    of its copy class (row_b, wire_b) holds `value_b`. Carries functions of witness values: treat it like the witness."""
    kind: int
    gate: int = 0
    constraint: int = 0
    wire: int = 0
    wire_b: int = 0
    row: int = 0
    row_b: int = 0
    value: int = 0
    value_b: int = 0

    def _c(self):
        return _WitnessFinding(self.kind, self.gate, self.constraint, self.wire, self.wire_b, 0, self.row, self.row_b, self.value, self.value_b)


def format_finding(pack, f, cap=256):
    """qpgpu_witness_finding_format: one line of text for a WitnessFinding, gates named as tools/pack_dump.py names them. Host only.
    Raises QpGpuError(-1) for a finding that does not fit the pack, (-5) when the line does not fit into cap bytes."""
    pw = np.ascontiguousarray(pack, dtype=np.uint64)
    buf = ctypes.create_string_buffer(cap)
    cf = f._c()
    rc = load_library().qpgpu_witness_finding_format(pw.ctypes.data, pw.size, ctypes.byref(cf), buf, cap)
    if rc:
        raise QpGpuError(rc, "witness_finding_format: " + ("the line does not fit: " + buf.value.decode() if rc == -5 else "the finding does not fit the pack"))
    return buf.value.decode()


class Circuit:
    """A circuit pack loaded on the GPU (constants/sigmas committed, workspace allocated)."""

    def __init__(self, gpu, pack_words, max_batch=1):
        self.gpu = gpu
        pw = np.ascontiguousarray(pack_words, dtype=np.uint64)
        h = ctypes.c_void_p()
        gpu._check(gpu.lib.qpgpu_circuit_load_batch(gpu.ctx, pw.ctypes.data, pw.size, max_batch, ctypes.byref(h)))
        self.h = h
        self.max_batch = max_batch
        self.num_public_inputs = int(pw[9])

    def scrub(self):
        """Overwrite every witness-derived device region of the workspace now."""
        self.gpu._check(self.gpu.lib.qpgpu_circuit_scrub(self.h))

    def prove_batch_dev(self, d_wires_list, public_inputs_list, outs=None):
        """Lockstep batch: one device witness and one public-input vector per proof; returns the list of proof bytes."""
        nb = len(d_wires_list)
        ptrs = (ctypes.c_void_p * nb)(*[_ptr(w) for w in d_wires_list])
        pis = [np.ascontiguousarray(p, dtype=np.uint64) for p in public_inputs_list]
        pip = (ctypes.c_void_p * nb)(*[p.ctypes.data for p in pis])
        size = self.proof_size()
        if outs is None:
            outs = [np.empty(size, dtype=np.uint8) for _ in range(nb)]
        op = (ctypes.c_void_p * nb)(*[o.ctypes.data for o in outs])
        lens = (ctypes.c_size_t * nb)()
        self.gpu._check(self.gpu.lib.qpgpu_prove_batch_dev(self.h, ptrs, nb, pip, op, size, lens))
        return [outs[i][:lens[i]].tobytes() for i in range(nb)]

    def close(self):
        if self.h:
            self.gpu.lib.qpgpu_circuit_free(self.h)
            self.h = None

    def proof_size(self):
        return self.gpu.lib.qpgpu_proof_size(self.h)

    def set_witness_check(self, on=True):
        """Make prove() return QPGPU_EUNSAT (-4) for a witness that violates a gate or copy constraint."""
        self.gpu._check(self.gpu.lib.qpgpu_circuit_set_witness_check(self.h, 1 if on else 0))

    def explain_witness(self, wires, public_inputs, max_rows=8, cap=4096):
        """qpgpu_circuit_explain_witness: (findings, failing_rows, copy_mismatches). findings: WitnessFinding list, the GATE findings
        of the first max_rows failing rows in (row, constraint) order, then COPY findings in (row, wire) order, `cap` at most;
        the two totals count everything there was. wires: a host array [num_wires, n], or a DeviceBuffer / device pointer."""
        on_device = not isinstance(wires, np.ndarray)
        if not on_device:
            wires = np.ascontiguousarray(wires, dtype=np.uint64)
        p = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        out = (_WitnessFinding * max(cap, 1))()
        n, rows, copies = ctypes.c_size_t(), ctypes.c_uint64(), ctypes.c_uint64()
        self.gpu._check(self.gpu.lib.qpgpu_circuit_explain_witness(self.h, _ptr(wires) if on_device else wires.ctypes.data, 1 if on_device else 0,
                                                                   p.ctypes.data, max_rows, 0, out, cap, ctypes.byref(n), ctypes.byref(rows), ctypes.byref(copies)))
        found = [WitnessFinding(f.kind, f.gate, f.constraint, f.wire, f.wire_b, f.row, f.row_b, f.value, f.value_b) for f in out[:n.value]]
        return found, rows.value, copies.value

    def set_quotient_fused(self, on=True):
        """Quotient stage: permutation terms and wire-local gates in one kernel where the gate list allows it (the default), or
        always the two kernels. Same proof bytes."""
        self.gpu._check(self.gpu.lib.qpgpu_circuit_set_quotient_fused(self.h, 1 if on else 0))

    def quotient_info(self):
        """(the switch, whether the one-pass kernel is what the next proof of this circuit runs)."""
        a, b = ctypes.c_int(), ctypes.c_int()
        self.gpu._check(self.gpu.lib.qpgpu_circuit_quotient_info(self.h, ctypes.byref(a), ctypes.byref(b)))
        return bool(a.value), bool(b.value)

    def quotient_pair_info(self):
        """(QPGPU_QUOTIENT_PAIR as read at load, whether one kernel serves both hash gates in the next proof of this circuit)."""
        a, b = ctypes.c_int(), ctypes.c_int()
        self.gpu._check(self.gpu.lib.qpgpu_circuit_quotient_pair_info(self.h, ctypes.byref(a), ctypes.byref(b)))
        return bool(a.value), bool(b.value)

    def set_blinding_seed(self, seed):
        """Zero-knowledge packs: fixes the salts of the next proof (reproducible bytes)."""
        self.gpu._check(self.gpu.lib.qpgpu_circuit_set_blinding_seed(self.h, seed))

    def constants_sigmas_cap(self, cap_height=4):
        out = np.empty((1 << cap_height, 4), dtype=np.uint64)
        self.gpu._check(self.gpu.lib.qpgpu_circuit_constants_sigmas_cap(self.h, out.ctypes.data, out.size))
        return out

    def witness_info(self):
        """(generator instances, dependency levels, caller-supplied cells) of the witness-generation plan."""
        a, b, c3 = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self.gpu._check(self.gpu.lib.qpgpu_witness_info(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c3)))
        return a.value, b.value, c3.value

    def gate_rows(self, gate_type):
        """The trace rows of a gate type (QPCP type codes: 4 PoseidonGate, 14 the Poseidon2 gate, ...)."""
        n = ctypes.c_size_t()
        self.gpu._check(self.gpu.lib.qpgpu_circuit_gate_rows(self.h, gate_type, None, 0, ctypes.byref(n)))
        rows = np.empty(n.value, dtype=np.uint32)
        self.gpu._check(self.gpu.lib.qpgpu_circuit_gate_rows(self.h, gate_type, rows.ctypes.data, rows.size, ctypes.byref(n)))
        return rows

    def witness_free_mask(self, num_wires, n):
        """uint8 [num_wires, n]: 1 where the caller supplies the cell (PartialWitness), 0 where generation writes it."""
        m = np.empty((num_wires, n), dtype=np.uint8)
        self.gpu._check(self.gpu.lib.qpgpu_witness_free_mask(self.h, m.ctypes.data, m.size))
        return m

    def generate_witness(self, wires, public_inputs):
        """Fills every generator- or copy-determined cell of a host wire matrix [num_wires, n]; returns the full matrix."""
        w = np.array(wires, dtype=np.uint64, order="C", copy=True)
        p = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        self.gpu._check(self.gpu.lib.qpgpu_generate_witness(self.h, w.ctypes.data, p.ctypes.data))
        return w

    def generate_witness_dev(self, d_wires, public_inputs, batch=1):
        """In place on `batch` device-resident wire matrices laid out back to back; public_inputs [batch, num_pis]."""
        p = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        self.gpu._check(self.gpu.lib.qpgpu_generate_witness_batch_dev(self.h, _ptr(d_wires), batch, p.ctypes.data))

    def generate_witness_partial_dev(self, cells, values, public_inputs, d_wires):
        """plonky2's PartialWitness as (cell = row * num_wires + wire, value) assignments -> full witness in d_wires.
        Raises QpGpuError(-4) when a target is set twice with different values."""
        cl = np.ascontiguousarray(cells, dtype=np.uint64); vl = np.ascontiguousarray(values, dtype=np.uint64)
        assert cl.shape == vl.shape
        p = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        self.gpu._check(self.gpu.lib.qpgpu_generate_witness_partial_dev(self.h, cl.ctypes.data, vl.ctypes.data, cl.size,
                                                                        p.ctypes.data, _ptr(d_wires)))

    def generate_witness_partial_batch_dev(self, cells, values, public_inputs, d_wires):
        """`batch` PartialWitnesses over one cell list: values [batch, count], public_inputs [batch, num_pis], d_wires batch
        matrices back to back. Returns the per-witness status list (0 or -4); never raises for an unsatisfied witness."""
        cl = np.ascontiguousarray(cells, dtype=np.uint64); vl = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, cl.size)
        p = None if public_inputs is None else np.ascontiguousarray(public_inputs, dtype=np.uint64)     # None: derived (witness_public_inputs_dev reads them)
        batch = vl.shape[0]
        status = (ctypes.c_int * batch)()
        rc = self.gpu.lib.qpgpu_generate_witness_partial_batch_dev(self.h, cl.ctypes.data, cl.size, vl.ctypes.data, None if p is None else p.ctypes.data, batch,
                                                                   _ptr(d_wires), status)
        if rc not in (0, -4):
            self.gpu._check(rc)
        return list(status)

    def generate_witness_partial_batch_blinded_dev(self, cells, values, public_inputs, d_wires, n_blinding, seeds=None):
        """The same with the LAST n_blinding cells drawn on the device (RandomValueGenerator targets of a zero-knowledge circuit):
        values [batch, count - n_blinding]; seeds: batch x 32 bytes for reproducible tests, None = OS entropy per witness."""
        cl = np.ascontiguousarray(cells, dtype=np.uint64)
        vl = np.ascontiguousarray(values, dtype=np.uint64)
        # (a circuit whose only assignments are its blinding cells: values [batch, 0])
        vl = vl.reshape(-1, cl.size - n_blinding) if cl.size > n_blinding else vl.reshape(vl.shape[0] if vl.ndim == 2 else 1, 0)
        p = None if public_inputs is None else np.ascontiguousarray(public_inputs, dtype=np.uint64)
        batch = vl.shape[0]
        sd = None
        if seeds is not None:
            sd = bytes(seeds)
            assert len(sd) == 32 * batch
        status = (ctypes.c_int * batch)()
        rc = self.gpu.lib.qpgpu_generate_witness_partial_batch_blinded_dev(self.h, cl.ctypes.data, cl.size, n_blinding, vl.ctypes.data, sd,
                                                                           None if p is None else p.ctypes.data, batch, _ptr(d_wires), status)
        if rc not in (0, -4):
            self.gpu._check(rc)
        return list(status)

    def witness_public_inputs_dev(self, d_wires, batch=1):
        """The public inputs of `batch` resident witnesses, [batch, num_public_inputs] (what plonky2's prove() reads out of the
        partition witness)."""
        out = np.empty((batch, self.num_public_inputs), dtype=np.uint64)
        self.gpu._check(self.gpu.lib.qpgpu_witness_public_inputs_dev(self.h, _ptr(d_wires), batch, out.ctypes.data))
        return out

    def witness_partial_prepare(self, cells, max_batch):
        cl = np.ascontiguousarray(cells, dtype=np.uint64)
        self.gpu._check(self.gpu.lib.qpgpu_witness_partial_prepare(self.h, cl.ctypes.data, cl.size, max_batch))

    def prove(self, wires, public_inputs):
        """wires: host array [num_wires, n]; returns proof bytes."""
        w = np.ascontiguousarray(wires, dtype=np.uint64)
        p = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        out = np.empty(self.proof_size(), dtype=np.uint8)
        ln = ctypes.c_size_t()
        self.gpu._check(self.gpu.lib.qpgpu_prove(self.h, w.ctypes.data, p.ctypes.data, out.ctypes.data, out.size, ctypes.byref(ln)))
        return out[:ln.value].tobytes()

    def prove_dev(self, d_wires, public_inputs, out=None):
        """wires resident in HBM (DeviceBuffer / torch tensor / raw pointer)."""
        p = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        if out is None:
            out = np.empty(self.proof_size(), dtype=np.uint8)
        ln = ctypes.c_size_t()
        self.gpu._check(self.gpu.lib.qpgpu_prove_dev(self.h, _ptr(d_wires), p.ctypes.data, out.ctypes.data, out.size, ctypes.byref(ln)))
        return out[:ln.value].tobytes()


ORACLE_VALUES, ORACLE_COEFFS, ORACLE_BLINDING, ORACLE_DEVICE_INPUT = 0, 1, 2, 4


class Verifier:
    """Host-side verifier of one circuit (include/qpgpu_verify.h): plonky2's VerifierCircuitData::verify over the circuit pack.
    circuit: a loaded Circuit whose constants/sigmas cap becomes the verifier data (without one the cap is rebuilt from the
    pack on the host). hasher: 0 Poseidon, 1 Poseidon2 (params None = the built-in qp-poseidon-core set)."""

    def __init__(self, pack_words, circuit=None, cap=None, hasher=0, params=None):
        lib = load_library()
        self.lib = lib
        pw = np.ascontiguousarray(pack_words, dtype=np.uint64)
        if cap is None and circuit is not None:
            cap = circuit.constants_sigmas_cap(int(pw[11]))
        cw = None if cap is None else np.ascontiguousarray(cap, dtype=np.uint64).reshape(-1)
        pr = None if params is None else np.ascontiguousarray(params, dtype=np.uint64)
        h = ctypes.c_void_p(); err = ctypes.create_string_buffer(200)
        rc = lib.qpgpu_verifier_create(pw.ctypes.data, pw.size, None if cw is None else cw.ctypes.data, 0 if cw is None else cw.size, hasher,
                                       None if pr is None else pr.ctypes.data, 0 if pr is None else pr.size, ctypes.byref(h), err)
        if rc:
            raise QpGpuError(rc, err.value.decode())
        self.h = h
        self.reason = ""

    def close(self):
        if self.h:
            self.lib.qpgpu_verifier_free(self.h); self.h = None

    def proof_size(self):
        return int(self.lib.qpgpu_verifier_proof_size(self.h))

    def verify(self, proof):
        """True when accepted; otherwise False and .reason says which check failed."""
        err = ctypes.create_string_buffer(200)
        b = bytes(proof)
        rc = self.lib.qpgpu_verifier_verify(self.h, b, len(b), err)
        self.reason = err.value.decode()
        return rc == 0

    HEAD_ON_DEVICE = 1      # QPGPU_VERIFY_HEAD_ON_DEVICE

    def verify_many(self, proofs, threads=0, gpu=None, device_head=False):
        """[accepted?] per proof, verified on up to `threads` host threads (0 = all cores); .reason names the first rejection.
        gpu: a QpGpu whose device runs the query rounds (qpgpu_verifier_verify_many_device; its hasher must be the verifier's);
        then .reasons holds the verifier's text for every proof ("" when accepted) and .results the codes. device_head (with
        gpu): the transcript, proof of work and quotient identity run on the device too (qpgpu_verifier_verify_many_device_ex,
        QPGPU_VERIFY_HEAD_ON_DEVICE); same verdicts and texts."""
        if device_head and gpu is None:
            raise ValueError("device_head=True needs gpu=")
        n = len(proofs)
        if n == 0:
            self.reasons, self.results = [], []
            return []
        bufs = [bytes(p) for p in proofs]
        ptrs = (ctypes.c_char_p * n)(*bufs)
        lens = (ctypes.c_size_t * n)(*[len(b) for b in bufs])
        res = (ctypes.c_int * n)()
        err = ctypes.create_string_buffer(200)
        if gpu is None:
            self.lib.qpgpu_verifier_verify_many(self.h, ptrs, lens, n, threads, res, err)
        else:
            rows = ctypes.create_string_buffer(200 * n)
            rc = self.lib.qpgpu_verifier_verify_many_device_ex(self.h, gpu.ctx, ptrs, lens, n, threads,
                                                               self.HEAD_ON_DEVICE if device_head else 0, res, rows, err)
            if rc not in (0, -6):
                raise QpGpuError(rc, err.value.decode())
            raw = rows.raw
            self.reasons = [raw[200 * i:200 * (i + 1)].split(b"\0", 1)[0].decode() for i in range(n)]
            self.results = list(res)
        self.reason = err.value.decode()
        return [r == 0 for r in res]


class ChallengerState(ctypes.Structure):
    """qpgpu_challenger: plonky2's Challenger as plain data (host only)."""
    _fields_ = [("sponge_state", ctypes.c_uint64 * 12), ("input_buffer", ctypes.c_uint64 * 8),
                ("output_buffer", ctypes.c_uint64 * 8), ("input_len", ctypes.c_uint32), ("output_len", ctypes.c_uint32)]


class Challenger:
    """gpu=None: the process-default hasher (first ABI); gpu=QpGpu: that context's hasher."""

    def __init__(self, gpu=None):
        self.lib = load_library()
        self.gpu = gpu
        self.state = ChallengerState()
        self.lib.qpgpu_challenger_init(ctypes.byref(self.state))

    def observe(self, xs):
        x = np.ascontiguousarray(xs, dtype=np.uint64).ravel()
        if self.gpu is None:
            self.lib.qpgpu_challenger_observe(ctypes.byref(self.state), x.ctypes.data, x.size)
        else:
            rc = self.lib.qpgpu_ctx_challenger_observe(self.gpu.ctx, ctypes.byref(self.state), x.ctypes.data, x.size)
            if rc != 0:
                raise QpGpuError(rc, "invalid challenger state")

    def get(self):
        if self.gpu is None:
            return int(self.lib.qpgpu_challenger_get(ctypes.byref(self.state)))
        v = ctypes.c_uint64()
        rc = self.lib.qpgpu_ctx_challenger_get(self.gpu.ctx, ctypes.byref(self.state), ctypes.byref(v))
        if rc != 0:
            raise QpGpuError(rc, "invalid challenger state")
        return int(v.value)

    def get_n(self, n):
        return [self.get() for _ in range(n)]


class _FriRange(ctypes.Structure):
    _fields_ = [("oracle", ctypes.c_uint32), ("first", ctypes.c_uint32), ("count", ctypes.c_uint32)]


class _FriBatch(ctypes.Structure):
    _fields_ = [("point", ctypes.c_uint64 * 2), ("num_ranges", ctypes.c_uint32), ("ranges", _FriRange * 8)]


class _FriParams(ctypes.Structure):
    _fields_ = [("rate_bits", ctypes.c_uint32), ("cap_height", ctypes.c_uint32), ("proof_of_work_bits", ctypes.c_uint32),
                ("num_query_rounds", ctypes.c_uint32), ("num_reduction_rounds", ctypes.c_uint32),
                ("reduction_arity_bits", ctypes.c_uint32 * 16)]


class PolyOracle:
    """A committed polynomial batch (plonky2 PolynomialBatch) resident on the GPU."""

    def __init__(self, gpu, polys, rate_bits=3, cap_height=4, coeffs=False, blinding=False, blinding_seed=0,
                 blinding_stream=0):
        self.gpu = gpu
        if isinstance(polys, np.ndarray):
            a = np.ascontiguousarray(polys, dtype=np.uint64)
            num_polys, n = a.shape
            ptr, flags = a.ctypes.data, 0
        else:                       # (device pointer, num_polys, n)
            dev, num_polys, n = polys
            ptr, flags = _ptr(dev), ORACLE_DEVICE_INPUT
        self.num_polys, self.n = num_polys, n
        self.degree_bits, self.rate_bits, self.cap_height = n.bit_length() - 1, rate_bits, cap_height
        assert 1 << self.degree_bits == n
        flags |= (ORACLE_COEFFS if coeffs else ORACLE_VALUES) | (ORACLE_BLINDING if blinding else 0)
        h = ctypes.c_void_p()
        gpu._check(gpu.lib.qpgpu_oracle_commit(gpu.ctx, ptr, num_polys, self.degree_bits, rate_bits, cap_height, flags,
                                               blinding_seed, blinding_stream, ctypes.byref(h)))
        self.h = h
        self.batch = None           # set by commit_batch: the oracle then answers through the batch entries

    @classmethod
    def commit_batch(cls, gpu, polys, rate_bits=3, cap_height=4, coeffs=False, blinding=False, blinding_seed=0, blinding_stream=0):
        """qpgpu_oracle_commit_batch: one oracle over the matrices of `batch` proofs. polys: a list of numpy arrays [num_polys, n]
        (or one array [batch, num_polys, n]), or a list of (device pointer, num_polys, n), back to back or separate allocations.
        With blinding, proof b's key is derived from blinding_seed + b (seed 0: fresh keys). cap / eval / open then take and return
        [batch, ...] arrays."""
        self = cls.__new__(cls)
        self.gpu = gpu
        if isinstance(polys, np.ndarray) or isinstance(polys[0], np.ndarray):
            keep = [np.ascontiguousarray(a, dtype=np.uint64) for a in polys]
            num_polys, n = keep[0].shape
            assert all(a.shape == (num_polys, n) for a in keep)
            ptrs, flags = [a.ctypes.data for a in keep], 0
        else:
            num_polys, n = polys[0][1], polys[0][2]
            assert all((q[1], q[2]) == (num_polys, n) for q in polys)
            ptrs, flags = [_ptr(q[0]) for q in polys], ORACLE_DEVICE_INPUT
        self.num_polys, self.n, self.batch = num_polys, n, len(ptrs)
        self.degree_bits, self.rate_bits, self.cap_height = n.bit_length() - 1, rate_bits, cap_height
        assert 1 << self.degree_bits == n
        flags |= (ORACLE_COEFFS if coeffs else ORACLE_VALUES) | (ORACLE_BLINDING if blinding else 0)
        h = ctypes.c_void_p()
        arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
        self.h = None
        gpu._check(gpu.lib.qpgpu_oracle_commit_batch(gpu.ctx, arr, len(ptrs), num_polys, self.degree_bits, rate_bits, cap_height, flags,
                                                     blinding_seed, blinding_stream, ctypes.byref(h)))
        self.h = h
        assert int(gpu.lib.qpgpu_oracle_batch(h)) == self.batch
        return self

    @classmethod
    def commit_sharded(cls, gpus, polys, rate_bits=3, cap_height=4, coeffs=False, blinding=False, blinding_seed=0, blinding_stream=0):
        """qpgpu_oracle_commit_sharded: one oracle whose leaves are split over the contexts `gpus` (QpGpu objects on any devices,
        a power of two of them, at most 2^rate_bits). gpus[0] is the home context: a (device pointer, num_polys, n) input lies on its
        device, and it is the context of every later call (the oracle's .gpu). cap / eval / read / open answer as an unsharded
        oracle's; .shards and .shard_range(g) say who holds what."""
        self = cls.__new__(cls)
        self.gpu, self.gpus = gpus[0], list(gpus)
        gpu = self.gpu
        if isinstance(polys, np.ndarray):
            a = np.ascontiguousarray(polys, dtype=np.uint64)
            num_polys, n = a.shape
            ptr, flags = a.ctypes.data, 0
        else:
            dev, num_polys, n = polys
            ptr, flags = _ptr(dev), ORACLE_DEVICE_INPUT
        self.num_polys, self.n, self.batch = num_polys, n, None
        self.degree_bits, self.rate_bits, self.cap_height = n.bit_length() - 1, rate_bits, cap_height
        assert 1 << self.degree_bits == n
        flags |= (ORACLE_COEFFS if coeffs else ORACLE_VALUES) | (ORACLE_BLINDING if blinding else 0)
        h = ctypes.c_void_p()
        ctxs = (ctypes.c_void_p * max(1, len(gpus)))(*[g.ctx for g in gpus])
        self.h = None
        gpu._check(gpu.lib.qpgpu_oracle_commit_sharded(ctxs, len(gpus), ptr, num_polys, self.degree_bits, rate_bits, cap_height, flags,
                                                       blinding_seed, blinding_stream, ctypes.byref(h)))
        self.h = h
        return self

    @property
    def shards(self):
        """Contexts the oracle's leaves are split over; 1 for an oracle of one context."""
        return int(self.gpu.lib.qpgpu_oracle_shards(self.h))

    def shard_range(self, shard):
        """(first leaf, number of leaves) of a shard."""
        first, num = ctypes.c_uint64(), ctypes.c_uint64()
        self.gpu._check(self.gpu.lib.qpgpu_oracle_shard_range(self.h, shard, ctypes.byref(first), ctypes.byref(num)))
        return int(first.value), int(num.value)

    def shard_device_ptrs(self, shard):
        """(LDE, digests) of a shard as integer addresses on the shard's device."""
        lde, dig = ctypes.c_void_p(), ctypes.c_void_p()
        self.gpu._check(self.gpu.lib.qpgpu_oracle_shard_device_ptrs(self.h, shard, ctypes.byref(lde), ctypes.byref(dig)))
        return lde.value, dig.value

    def strides(self):
        """Words between two proofs' (coefficients, LDEs, digests); (0, 0, 0) for an oracle of one proof."""
        v = [ctypes.c_uint64() for _ in range(3)]
        self.gpu._check(self.gpu.lib.qpgpu_oracle_strides(self.h, *[ctypes.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def close(self):
        if self.h:
            self.gpu.lib.qpgpu_oracle_free(self.h)
            self.h = None

    def cap(self):
        if self.batch is not None:
            out = np.empty((self.batch, 4 << self.cap_height), dtype=np.uint64)
            self.gpu._check(self.gpu.lib.qpgpu_oracle_cap(self.h, out.ctypes.data, out.size))
            return out
        out = np.empty((1 << self.cap_height, 4), dtype=np.uint64)
        self.gpu._check(self.gpu.lib.qpgpu_oracle_cap(self.h, out.ctypes.data, out.size))
        return out

    def eval(self, point, first=0, count=None):
        """Evaluations at an extension point (a, b): array [count, 2]."""
        count = self.num_polys - first if count is None else count
        if self.batch is not None:              # points [batch, 2] -> [batch, count, 2]
            pt = np.ascontiguousarray(np.array(point, dtype=np.uint64).reshape(self.batch, 2))
            out = np.empty((self.batch, count, 2), dtype=np.uint64)
            self.gpu._check(self.gpu.lib.qpgpu_oracle_eval_batch(self.h, pt.ctypes.data, first, count, out.ctypes.data))
            return out
        pt = np.array(point, dtype=np.uint64)
        out = np.empty((count, 2), dtype=np.uint64)
        self.gpu._check(self.gpu.lib.qpgpu_oracle_eval(self.h, pt.ctypes.data, first, count, out.ctypes.data))
        return out

    def read(self, lde=False, first=0, count=None):
        count = self.num_polys - first if count is None else count
        out = np.empty((count, self.n << (self.rate_bits if lde else 0)), dtype=np.uint64)
        self.gpu._check(self.gpu.lib.qpgpu_oracle_read(self.h, 1 if lde else 0, first, count, out.ctypes.data))
        return out

    @property
    def leaf_width(self):
        """Words of a Merkle leaf: num_polys, + 4 salt words for a blinded oracle."""
        return int(self.gpu.lib.qpgpu_oracle_leaf_width(self.h))

    def open(self, indices, rows=True, paths=True):
        """MerkleTree::prove at leaf indices: (rows [n, leaf_width], paths [n, degree_bits + rate_bits - cap_height, 4]); an
        output that is not asked for comes back as None."""
        plen = self.degree_bits + self.rate_bits - self.cap_height
        if self.batch is not None:              # indices [batch, n] -> rows [batch, n, leaf_width], paths [batch, n, plen, 4]
            idx = np.ascontiguousarray(np.array(indices, dtype=np.uint64).reshape(self.batch, -1))
            n = idx.shape[1]
            r = np.zeros((self.batch, n, self.leaf_width), dtype=np.uint64) if rows else None
            p = np.zeros((self.batch, n, plen, 4), dtype=np.uint64) if paths else None
            self.gpu._check(self.gpu.lib.qpgpu_oracle_open_batch(self.h, idx.ctypes.data if n else None, n,
                                                                 r.ctypes.data if rows else None, p.ctypes.data if paths else None))
            return r, p
        idx = np.ascontiguousarray(indices, dtype=np.uint64).ravel()
        r = np.empty((idx.size, self.leaf_width), dtype=np.uint64) if rows else None
        p = np.empty((idx.size, plen, 4), dtype=np.uint64) if paths else None
        self.gpu._check(self.gpu.lib.qpgpu_oracle_open(self.h, idx.ctypes.data if idx.size else None, idx.size,
                                                       r.ctypes.data if rows else None, p.ctypes.data if paths else None))
        return r, p


STAGE_ERR_CAP = 256


def stage_header_words(pack_words):
    """The pack without its constants/sigmas value block: header .. k_is, circuit_digest, then the trailers — the short form
    of the words qpgpu_stage_plan_create takes (the values are in the caller's constants/sigmas oracle)."""
    pw = np.ascontiguousarray(pack_words, dtype=np.uint64)
    h = pack_header(pw)
    end = 18 + h["num_arity_rounds"] + 8 * h["num_gates"] + h["num_routed_wires"] + 4
    ncs = h["num_selectors"] + h["num_constants"] + h["num_routed_wires"]
    return np.concatenate([pw[:end], pw[end + (ncs << h["degree_bits"]):]])


class StagePlan:
    """qpgpu_stage_plan: stages s5 (partial products) and s6 (quotient) of the stage flow on the device, for one circuit.
    pack_words: the full pack or stage_header_words(pack); cs_oracle: the PolyOracle of the constants/sigmas values (no
    blinding), which must stay open as long as the plan."""

    @classmethod
    def create_sharded(cls, gpu, pack_words, cs_oracle):
        """qpgpu_stage_plan_create_sharded: a plan over a constants/sigmas oracle from PolyOracle.commit_sharded; gpu is its home
        context. quotient() then takes wire and Z/partial-products oracles sharded over the same contexts."""
        return cls(gpu, pack_words, cs_oracle, sharded=True)

    def __init__(self, gpu, pack_words, cs_oracle, max_batch=None, sharded=False):
        """max_batch: None = qpgpu_stage_plan_create (one proof); a number = qpgpu_stage_plan_create_batch, a workspace for that
        many proofs in lockstep (partial_products_batch, quotient_batch). sharded=True: qpgpu_stage_plan_create_sharded (one proof)."""
        self.gpu, self.cs_oracle = gpu, cs_oracle
        pw = np.ascontiguousarray(pack_words, dtype=np.uint64)
        h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(STAGE_ERR_CAP)
        cs = cs_oracle.h if cs_oracle is not None else None
        if sharded:
            assert max_batch is None, "a sharded plan takes one proof"
            rc = gpu.lib.qpgpu_stage_plan_create_sharded(gpu.ctx, pw.ctypes.data, pw.size, cs, ctypes.byref(h), err)
        elif max_batch is None:
            rc = gpu.lib.qpgpu_stage_plan_create(gpu.ctx, pw.ctypes.data, pw.size, cs, ctypes.byref(h), err)
        else:
            rc = gpu.lib.qpgpu_stage_plan_create_batch(gpu.ctx, pw.ctypes.data, pw.size, cs, max_batch, ctypes.byref(h), err)
        if rc != 0:
            raise QpGpuError(rc, err.value.decode())
        self.h = h
        self.max_batch = int(gpu.lib.qpgpu_stage_plan_max_batch(h))
        self.shards = int(gpu.lib.qpgpu_stage_plan_shards(h))      # contexts the plan's oracles are split over; 1: a plan on one context
        v = [ctypes.c_uint() for _ in range(4)]
        fused = ctypes.c_int()
        gpu._check(gpu.lib.qpgpu_stage_plan_info(h, *[ctypes.byref(x) for x in v], ctypes.byref(fused)))
        self.degree_bits, self.num_challenges, self.num_partial_products, self.quotient_degree_factor = [int(x.value) for x in v]
        self.fused_selected = bool(fused.value)
        self.n = 1 << self.degree_bits
        self.num_zs_pp = self.num_challenges * (1 + self.num_partial_products)
        self.num_quotient = self.num_challenges * self.quotient_degree_factor

    def close(self):
        if self.h:
            self.gpu.lib.qpgpu_stage_plan_free(self.h)
            self.h = None

    def _challenges(self, xs):
        a = np.ascontiguousarray(xs, dtype=np.uint64).ravel()
        assert a.size == self.num_challenges
        return a

    def partial_products(self, wires, betas, gammas):
        """wires: the witness matrix as a numpy array [num_wires, n] (host) or a DeviceBuffer / device pointer. Returns a
        DeviceBuffer of num_zs_pp columns of n values: PolyOracle(gpu, (buf, plan.num_zs_pp, plan.n), ...) commits it."""
        b, g = self._challenges(betas), self._challenges(gammas)
        if isinstance(wires, np.ndarray):
            w = np.ascontiguousarray(wires, dtype=np.uint64)
            ptr, on_dev = w.ctypes.data, 0
        else:
            ptr, on_dev = _ptr(wires), 1
        out = self.gpu.alloc(self.num_zs_pp * self.n * 8)
        rc = self.gpu.lib.qpgpu_stage_partial_products(self.h, ptr, on_dev, b.ctypes.data, g.ctypes.data, out.ptr)
        if rc != 0:
            out.free(scrub=True)
            self.gpu._check(rc)
        return out

    def quotient(self, wires_oracle, zs_pp_oracle, betas, gammas, alphas, public_inputs_hash):
        """Returns a DeviceBuffer of num_quotient columns of n coefficients:
        PolyOracle(gpu, (buf, plan.num_quotient, plan.n), coeffs=True, ...) commits it. QpGpuError -4 for a witness that does not
        satisfy the circuit. On a plan from create_sharded the two oracles are sharded ones (PolyOracle.commit_sharded over the
        contexts of the plan's cs_oracle); the buffer is on the home context and holds the same words."""
        b, g, a = self._challenges(betas), self._challenges(gammas), self._challenges(alphas)
        pih = np.ascontiguousarray(public_inputs_hash, dtype=np.uint64).ravel()
        assert pih.size == 4
        out = self.gpu.alloc(self.num_quotient * self.n * 8)
        rc = self.gpu.lib.qpgpu_stage_quotient(self.h, wires_oracle.h, zs_pp_oracle.h, b.ctypes.data, g.ctypes.data, a.ctypes.data,
                                               pih.ctypes.data, out.ptr)
        if rc != 0:
            out.free(scrub=True)
            self.gpu._check(rc)
        return out


    def _challenges_batch(self, xs, batch, width=None):
        a = np.ascontiguousarray(xs, dtype=np.uint64)
        assert a.size == batch * (self.num_challenges if width is None else width)
        return a

    def partial_products_batch(self, wires, betas, gammas):
        """s5 for a lockstep batch. wires: a list of numpy arrays [num_wires, n] (host) or of DeviceBuffers / device pointers (back
        to back or separate). betas, gammas: [batch, num_challenges]. Returns a DeviceBuffer [batch][num_zs_pp][n], dense."""
        batch = len(wires)
        b, g = self._challenges_batch(betas, batch), self._challenges_batch(gammas, batch)
        if isinstance(wires[0], np.ndarray):
            keep = [np.ascontiguousarray(w, dtype=np.uint64) for w in wires]
            ptrs, on_dev = [w.ctypes.data for w in keep], 0
        else:
            ptrs, on_dev = [_ptr(w) for w in wires], 1
        arr = (ctypes.c_void_p * batch)(*ptrs)
        out = self.gpu.alloc(batch * self.num_zs_pp * self.n * 8)
        rc = self.gpu.lib.qpgpu_stage_partial_products_batch(self.h, arr, batch, on_dev, b.ctypes.data, g.ctypes.data, out.ptr)
        if rc != 0:
            out.free(scrub=True)
            self.gpu._check(rc)
        return out

    def quotient_batch(self, wires_oracle, zs_pp_oracle, batch, betas, gammas, alphas, public_inputs_hashes):
        """s6 for a lockstep batch: the two oracles hold `batch` proofs each (PolyOracle.commit_batch). betas, gammas, alphas:
        [batch, num_challenges]; public_inputs_hashes [batch, 4]. Returns a DeviceBuffer [batch][num_quotient][n] of coefficients.
        QpGpuError -4 concerns the whole batch; the message names the proof."""
        b, g, a = (self._challenges_batch(x, batch) for x in (betas, gammas, alphas))
        pih = self._challenges_batch(public_inputs_hashes, batch, 4)
        out = self.gpu.alloc(batch * self.num_quotient * self.n * 8)
        rc = self.gpu.lib.qpgpu_stage_quotient_batch(self.h, wires_oracle.h, zs_pp_oracle.h, batch, b.ctypes.data, g.ctypes.data,
                                                     a.ctypes.data, pih.ctypes.data, out.ptr)
        if rc != 0:
            out.free(scrub=True)
            self.gpu._check(rc)
        return out


def _fri_args(oracles, batches, reduction_arity_bits, rate_bits, cap_height, proof_of_work_bits, num_query_rounds):
    hs = (ctypes.c_void_p * len(oracles))(*[o.h for o in oracles])
    bs = (_FriBatch * len(batches))()
    for b, (point, ranges) in zip(bs, batches):
        if np.ndim(point) == 1:     # the batch entries do not read this field: their points travel in an array of their own
            b.point[0], b.point[1] = int(point[0]), int(point[1])
        b.num_ranges = len(ranges)
        for r, (o, f, cnt) in zip(b.ranges, ranges):
            r.oracle, r.first, r.count = o, f, cnt
    prm = _FriParams(rate_bits, cap_height, proof_of_work_bits, num_query_rounds, len(reduction_arity_bits))
    for i, a in enumerate(reduction_arity_bits):
        prm.reduction_arity_bits[i] = a
    return hs, bs, prm


def fri_prove(gpu, oracles, batches, challenger, reduction_arity_bits, rate_bits=3, cap_height=4, proof_of_work_bits=16,
              num_query_rounds=28):
    """PolynomialBatch::prove_openings. batches: [(point(a, b), [(oracle, first, count), ...]), ...]; challenger is
    advanced in place. Returns the FriProof bytes."""
    hs, bs, prm = _fri_args(oracles, batches, reduction_arity_bits, rate_bits, cap_height, proof_of_work_bits, num_query_rounds)
    size = gpu.lib.qpgpu_fri_proof_size(hs, len(oracles), ctypes.byref(prm))
    if size == 0:
        raise QpGpuError(-1, "fri_prove: bad oracles or FRI parameters")
    out = np.empty(size, dtype=np.uint8)
    ln = ctypes.c_size_t()
    gpu._check(gpu.lib.qpgpu_fri_prove(gpu.ctx, hs, len(oracles), ctypes.byref(bs), len(batches), ctypes.byref(prm),
                                       ctypes.byref(challenger.state), out.ctypes.data, out.size, ctypes.byref(ln)))
    return out[:ln.value].tobytes()


def fri_prove_batch(gpu, oracles, batches, challengers, reduction_arity_bits, rate_bits=3, cap_height=4, proof_of_work_bits=16,
                    num_query_rounds=28):
    """qpgpu_fri_prove_batch: fri_prove for len(challengers) proofs in lockstep. oracles hold that many proofs (PolyOracle.commit_batch)
    or one shared by all; batches: [(points [batch, 2], ranges), ...]; the challengers are advanced in place. Returns a list of
    FriProof bytes."""
    nb = len(challengers)
    hs, bs, prm = _fri_args(oracles, batches, reduction_arity_bits, rate_bits, cap_height, proof_of_work_bits, num_query_rounds)
    pts = np.ascontiguousarray(np.array([np.array(pt, dtype=np.uint64).reshape(nb, 2) for pt, _ in batches], dtype=np.uint64))
    size = gpu.lib.qpgpu_fri_proof_size(hs, len(oracles), ctypes.byref(prm))
    if size == 0:
        raise QpGpuError(-1, "fri_prove: bad oracles or FRI parameters")
    states = (ChallengerState * nb)()
    for i, ch in enumerate(challengers):
        ctypes.memmove(ctypes.byref(states[i]), ctypes.byref(ch.state), ctypes.sizeof(ChallengerState))
    outs = [np.empty(size, dtype=np.uint8) for _ in range(nb)]
    optr = (ctypes.c_void_p * nb)(*[o.ctypes.data for o in outs])
    lens = (ctypes.c_size_t * nb)()
    gpu._check(gpu.lib.qpgpu_fri_prove_batch(gpu.ctx, hs, len(oracles), ctypes.byref(bs), len(batches), pts.ctypes.data, nb,
                                             ctypes.byref(prm), ctypes.byref(states), optr, size, lens))
    for i, ch in enumerate(challengers):
        ctypes.memmove(ctypes.byref(ch.state), ctypes.byref(states[i]), ctypes.sizeof(ChallengerState))
    return [outs[i][:lens[i]].tobytes() for i in range(nb)]


def fri_grind_batch(gpu, challengers, proof_of_work_bits):
    """qpgpu_fri_grind_batch: the minimum nonces of len(challengers) transcripts in one search; none is advanced."""
    nb = len(challengers)
    states = (ChallengerState * nb)()
    for i, ch in enumerate(challengers):
        ctypes.memmove(ctypes.byref(states[i]), ctypes.byref(ch.state), ctypes.sizeof(ChallengerState))
    nonces = (ctypes.c_uint64 * nb)()
    gpu._check(gpu.lib.qpgpu_fri_grind_batch(gpu.ctx, ctypes.byref(states), nb, proof_of_work_bits, nonces))
    return [int(x) for x in nonces]


def fri_grind(gpu, challenger, proof_of_work_bits):
    """The minimum proof-of-work nonce for a transcript in `challenger`'s state (qpgpu_fri_grind); the challenger is not advanced."""
    nonce = ctypes.c_uint64()
    gpu._check(gpu.lib.qpgpu_fri_grind(gpu.ctx, ctypes.byref(challenger.state), proof_of_work_bits, ctypes.byref(nonce)))
    return int(nonce.value)


class FriSession:
    """qpgpu_fri_session: the FRI opening proof one step at a time; the caller keeps the transcript. Arguments as fri_prove's, with
    the FRI alpha in place of the challenger. A context manager; the oracles must stay open as long as the session.

        with FriSession(gpu, oracles, batches, ch.get_n(2), arity_bits, rate_bits=3, cap_height=4) as fs:
            for _ in arity_bits:
                ch.observe(fs.round_commit()); fs.round_fold(ch.get_n(2))
            final = fs.final_poly(); ch.observe(final)
            nonce = fri_grind(gpu, ch, pow_bits); ch.observe([nonce]); ch.get()
            queries = fs.open([ch.get() % fs.lde_size for _ in range(num_query_rounds)])"""

    def __init__(self, gpu, oracles, batches, alpha, reduction_arity_bits, rate_bits=3, cap_height=4, batch=None):
        """batch: None = qpgpu_fri_begin. A number = qpgpu_fri_begin_batch, that many proofs in lockstep: alpha is [batch, 2], each
        opening batch's point [batch, 2]; round_commit returns [batch, cap_words], round_fold takes [batch, 2], final_poly returns
        [batch, final_len, 2], open takes [batch, n] indices and returns a list of bytes, one per proof."""
        self.gpu, self.oracles, self.batch = gpu, list(oracles), batch
        hs, bs, prm = _fri_args(oracles, batches, reduction_arity_bits, rate_bits, cap_height, 0, 0)
        h = ctypes.c_void_p()
        if batch is None:
            a = np.array([int(alpha[0]), int(alpha[1])], dtype=np.uint64)
            gpu._check(gpu.lib.qpgpu_fri_begin(gpu.ctx, hs, len(oracles), ctypes.byref(bs), len(batches), ctypes.byref(prm), a.ctypes.data,
                                               ctypes.byref(h)))
        else:
            a = np.ascontiguousarray(np.array(alpha, dtype=np.uint64).reshape(batch, 2))
            pts = np.ascontiguousarray(np.array([np.array(pt, dtype=np.uint64).reshape(batch, 2) for pt, _ in batches], dtype=np.uint64))
            gpu._check(gpu.lib.qpgpu_fri_begin_batch(gpu.ctx, hs, len(oracles), ctypes.byref(bs), len(batches), pts.ctypes.data, batch,
                                                     ctypes.byref(prm), a.ctypes.data, ctypes.byref(h)))
            assert int(gpu.lib.qpgpu_fri_session_batch(h)) == batch
        self.h = h
        self.cap_height, self.arity_bits = cap_height, list(reduction_arity_bits)
        self.lde_size = 1 << (oracles[0].degree_bits + rate_bits)
        self.final_len = 1 << (oracles[0].degree_bits - sum(self.arity_bits))
        self.query_size = int(gpu.lib.qpgpu_fri_query_size(h))

    def close(self):
        if self.h:
            self.gpu.lib.qpgpu_fri_session_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def round_commit(self):
        """Commit the current layer: its cap, [2^cap_height, 4]."""
        shape = (1 << self.cap_height, 4) if self.batch is None else (self.batch, 4 << self.cap_height)
        cap = np.empty(shape, dtype=np.uint64)
        self.gpu._check(self.gpu.lib.qpgpu_fri_round_commit(self.h, cap.ctypes.data, cap.size))
        return cap

    def round_fold(self, beta):
        b = np.ascontiguousarray(np.array(beta, dtype=np.uint64).reshape(self.batch or 1, 2))
        self.gpu._check(self.gpu.lib.qpgpu_fri_round_fold(self.h, b.ctypes.data))

    def final_poly(self):
        """The final polynomial's coefficients, [final_len, 2]."""
        out = np.empty((self.final_len, 2) if self.batch is None else (self.batch, self.final_len, 2), dtype=np.uint64)
        n = ctypes.c_size_t()
        self.gpu._check(self.gpu.lib.qpgpu_fri_final_poly(self.h, out.ctypes.data, out.size, ctypes.byref(n)))
        assert n.value == self.final_len
        return out

    def open(self, indices):
        """The FriQueryRound bytes of each index, back to back (query_size bytes each)."""
        if self.batch is not None:
            idx = np.ascontiguousarray(np.array(indices, dtype=np.uint64).reshape(self.batch, -1))
            n, per = idx.shape[1], idx.shape[1] * self.query_size
            out = np.empty(max(1, self.batch * per), dtype=np.uint8)
            ln = ctypes.c_size_t()
            self.gpu._check(self.gpu.lib.qpgpu_fri_open(self.h, idx.ctypes.data if n else None, n, out.ctypes.data, self.batch * per,
                                                        ctypes.byref(ln)))
            assert ln.value == self.batch * per
            return [out[b * per:(b + 1) * per].tobytes() for b in range(self.batch)]
        idx = np.ascontiguousarray(indices, dtype=np.uint64).ravel()
        out = np.empty(max(1, idx.size * self.query_size), dtype=np.uint8)
        ln = ctypes.c_size_t()
        self.gpu._check(self.gpu.lib.qpgpu_fri_open(self.h, idx.ctypes.data if idx.size else None, idx.size, out.ctypes.data,
                                                    idx.size * self.query_size, ctypes.byref(ln)))
        return out[:ln.value].tobytes()


class _FriOracleShape(ctypes.Structure):
    _fields_ = [("num_polys", ctypes.c_uint32), ("blinded", ctypes.c_uint32)]


class _FriInstance(ctypes.Structure):
    _fields_ = [("degree_bits", ctypes.c_uint32), ("num_oracles", ctypes.c_uint32), ("oracles", ctypes.POINTER(_FriOracleShape)),
                ("num_batches", ctypes.c_uint32), ("batches", ctypes.POINTER(_FriBatch)), ("params", _FriParams)]


class FriVerifier:
    """qpgpu_fri_verifier (include/qpgpu_verify.h): fri::verifier::verify_fri_proof for the proofs fri_prove / FriSession make.
    oracles: [(num_polys, blinded), ...]; batches: one list of (oracle, first, count) per opening point, as fri_prove's without
    the points. hasher / params as Verifier's. Host only except verify_many(gpu=...)."""

    def __init__(self, degree_bits, oracles, batches, reduction_arity_bits, rate_bits=3, cap_height=4, proof_of_work_bits=16,
                 num_query_rounds=28, hasher=0, params=None):
        self.lib = load_library()
        shapes = (_FriOracleShape * max(1, len(oracles)))(*[_FriOracleShape(int(n), int(bool(b))) for n, b in oracles])
        _, bs, prm = _fri_args([], [((0, 0), r) for r in batches], reduction_arity_bits, rate_bits, cap_height, proof_of_work_bits,
                               num_query_rounds)
        inst = _FriInstance(degree_bits, len(oracles), shapes, len(batches), bs, prm)
        pr = None if params is None else np.ascontiguousarray(params, dtype=np.uint64)
        h = ctypes.c_void_p(); err = ctypes.create_string_buffer(200)
        rc = self.lib.qpgpu_fri_verifier_create(ctypes.byref(inst), hasher, None if pr is None else pr.ctypes.data,
                                                0 if pr is None else pr.size, ctypes.byref(h), err)
        if rc:
            raise QpGpuError(rc, err.value.decode())
        self.h = h
        self.num_oracles, self.num_batches, self.num_rounds = len(oracles), len(batches), len(reduction_arity_bits)
        self.num_queries, self.cap_words = num_query_rounds, 4 << cap_height
        self.reason, self.code = "", 0

    def close(self):
        if self.h:
            self.lib.qpgpu_fri_verifier_free(self.h); self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def proof_size(self):
        return int(self.lib.qpgpu_fri_verifier_proof_size(self.h))

    def num_openings(self):
        return int(self.lib.qpgpu_fri_verifier_num_openings(self.h))

    def challenges(self, challenger, proof):
        """Challenger::fri_challenges: (alpha (a, b), betas [(a, b)], proof-of-work response, query indices); `challenger`
        (the transcript after the openings) is advanced in place, under the verifier's hasher."""
        b = bytes(proof)
        alpha = np.zeros(2, dtype=np.uint64); betas = np.zeros((max(1, self.num_rounds), 2), dtype=np.uint64)
        idx = np.zeros(self.num_queries, dtype=np.uint64); powr = ctypes.c_uint64(); err = ctypes.create_string_buffer(200)
        rc = self.lib.qpgpu_fri_verifier_challenges(self.h, ctypes.byref(challenger.state), b, len(b), alpha.ctypes.data, betas.ctypes.data,
                                                    ctypes.byref(powr), idx.ctypes.data, err)
        if rc:
            raise QpGpuError(rc, err.value.decode())
        return ((int(alpha[0]), int(alpha[1])), [(int(x[0]), int(x[1])) for x in betas[:self.num_rounds]], int(powr.value),
                [int(x) for x in idx])

    @staticmethod
    def _words(x, shape):
        return np.ascontiguousarray(np.array(x, dtype=np.uint64).reshape(shape))

    def verify(self, caps, points, openings, alpha, betas, pow_response, indices, proof):
        """qpgpu_fri_verify. caps: one array of 4 << cap_height words per oracle; points: [(a, b)] per batch; openings:
        [num_openings, 2]. True when accepted; else False with .code (-6 rejected, -1 the caller's own values refused) and
        .reason."""
        keep = [self._words(cp, -1) for cp in caps]
        assert len(keep) == self.num_oracles and all(k.size == self.cap_words for k in keep)
        cptr = (ctypes.c_void_p * max(1, len(keep)))(*[k.ctypes.data for k in keep])
        pts, ops = self._words(points, (self.num_batches, 2)), self._words(openings, (self.num_openings(), 2))
        a, bt = self._words(alpha, 2), self._words(betas if self.num_rounds else [0, 0], (max(1, self.num_rounds), 2))
        idx = self._words(indices, self.num_queries)
        b = bytes(proof); err = ctypes.create_string_buffer(200)
        self.code = self.lib.qpgpu_fri_verify(self.h, cptr, pts.ctypes.data, ops.ctypes.data, a.ctypes.data, bt.ctypes.data, int(pow_response),
                                              idx.ctypes.data, b, len(b), err)
        self.reason = err.value.decode()
        return self.code == 0

    def verify_many(self, caps, points, openings, alphas, betas, pow_responses, indices, proofs, gpu=None, cap_counts=None):
        """qpgpu_fri_verify_many_device on gpu's device (gpu=None: one qpgpu_fri_verify per proof on the host). caps: per oracle
        [cap_words] (shared by all proofs) or [count, cap_words]; points [num_batches, count, 2]; openings [count, num_openings, 2];
        alphas [count, 2]; betas [count, rounds, 2]; pow_responses [count]; indices [count, num_queries]. Returns [accepted?];
        .results the codes, .reasons the texts ("" when accepted), .code / .reason the call's."""
        n = len(proofs)
        keep = [self._words(cp, -1) for cp in caps]
        counts = list(cap_counts) if cap_counts is not None else [k.size // self.cap_words for k in keep]
        pts = self._words(points, (self.num_batches, n, 2)) if n else np.zeros(2, dtype=np.uint64)
        ops = self._words(openings, (n, self.num_openings(), 2)) if n else np.zeros(2, dtype=np.uint64)
        al = self._words(alphas, (n, 2)) if n else np.zeros(2, dtype=np.uint64)
        bt = self._words(betas, (n, self.num_rounds, 2)) if n and self.num_rounds else np.zeros(2, dtype=np.uint64)
        pw = self._words(pow_responses, n) if n else np.zeros(1, dtype=np.uint64)
        idx = self._words(indices, (n, self.num_queries)) if n else np.zeros(1, dtype=np.uint64)
        if gpu is None:
            self.results, self.reasons = [], []
            for i in range(n):
                own = [k.reshape(-1, self.cap_words)[i if c != 1 else 0] for k, c in zip(keep, counts)]
                self.verify(own, pts[:, i], ops[i], al[i], bt[i] if self.num_rounds else None, int(pw[i]), idx[i], proofs[i])
                self.results.append(self.code); self.reasons.append(self.reason)
            bad = [i for i, r in enumerate(self.results) if r]
            self.code = self.results[bad[0]] if bad else 0
            self.reason = "proof %d: %s" % (bad[0], self.reasons[bad[0]]) if bad else ""
            return [r == 0 for r in self.results]
        bufs = [bytes(p) for p in proofs]
        ptrs = (ctypes.c_char_p * max(1, n))(*bufs)
        lens = (ctypes.c_size_t * max(1, n))(*[len(b) for b in bufs])
        cptr = (ctypes.c_void_p * max(1, len(keep)))(*[k.ctypes.data for k in keep])
        cc = (ctypes.c_uint32 * max(1, len(keep)))(*counts)
        res = (ctypes.c_int * max(1, n))()
        rows = ctypes.create_string_buffer(200 * max(1, n)); err = ctypes.create_string_buffer(200)
        self.code = self.lib.qpgpu_fri_verify_many_device(self.h, gpu.ctx, n, cptr, cc, pts.ctypes.data, ops.ctypes.data, al.ctypes.data,
                                                          bt.ctypes.data, pw.ctypes.data, idx.ctypes.data, ptrs, lens, res, rows, err)
        self.reason = err.value.decode()
        raw = rows.raw
        self.reasons = [raw[200 * i:200 * (i + 1)].split(b"\0", 1)[0].decode() for i in range(n)]
        self.results = list(res)[:n]
        return [r == 0 for r in self.results]


class ResidueHit(ctypes.Structure):
    """qpgpu_residue_hit: one needle word found in a buffer the library owns."""
    _fields_ = [("word", ctypes.c_uint64), ("region", ctypes.c_uint32), ("pinned", ctypes.c_uint32),
                ("offset_words", ctypes.c_uint64), ("alloc_bytes", ctypes.c_uint64)]

    def as_dict(self):
        name = load_library().qpgpu_residue_region_name(self.region)
        return {"word": self.word, "region": name.decode() if name else None, "pinned": bool(self.pinned),
                "offset_words": self.offset_words, "alloc_bytes": self.alloc_bytes}


RESIDUE_MAX_NEEDLES = 16


def residue_regions():
    """The stable region names of the residue audit, by region number."""
    lib, out = load_library(), []
    while True:
        name = lib.qpgpu_residue_region_name(len(out))
        if name is None:
            return out
        out.append(name.decode())


def _residue_mask(regions):
    """None -> 0 (the library's default: every region that can hold witness-derived words); an int is passed through; names are looked up."""
    if regions is None:
        return 0
    if isinstance(regions, int):
        return regions
    names = residue_regions()
    return sum(1 << names.index(r) for r in set(regions))


_NO_REGION = 0xFFFFFFFF


def _blank_hits(cap):
    """The library writes the hits it recorded (at most 64 per device buffer) and leaves the rest of the array as it was: entries
    marked with a region no buffer has are the ones it did not write."""
    first = (ResidueHit * max(cap, 1))()
    for h in first:
        h.region = _NO_REGION
    return first


def _written_hits(first, cap):
    out = []
    for i in range(cap):
        if first[i].region == _NO_REGION:
            break
        out.append(first[i].as_dict())
    return out


def _residue_call(fn, handle, needles, regions, cap):
    nd = np.ascontiguousarray(needles, dtype=np.uint64)
    hits, nbytes = ctypes.c_uint64(), ctypes.c_uint64()
    first = _blank_hits(cap)
    rc = fn(handle, nd.ctypes.data, nd.size, _residue_mask(regions), ctypes.byref(hits), first, cap, ctypes.byref(nbytes))
    return rc, hits.value, _written_hits(first, cap), nbytes.value


class ProvingPool:
    """Several proofs of one circuit in flight on one GPU (qpgpu_pool_*): worker threads, streams and circuit copies live
    inside the library."""

    def __init__(self, pack_words, workers=4, device=0, max_batch=1, devices=None, host_witness=False):
        """devices: a list of HIP devices (one entry may repeat) -> qpgpu_pool_create_multi with `workers` workers on each."""
        self.lib = load_library()
        pw = np.ascontiguousarray(pack_words, dtype=np.uint64)
        h = ctypes.c_void_p()
        devs = [device] if devices is None else list(devices)
        arr = (ctypes.c_int * len(devs))(*devs)
        rc = self.lib.qpgpu_pool_create_multi(arr, len(devs), pw.ctypes.data, pw.size, workers, max_batch, 1 if host_witness else 0, ctypes.byref(h))
        if rc != 0:
            raise QpGpuError(rc, "qpgpu_pool_create failed")
        self.h = h
        self._keep = {}
        # the workers write into the callers' output buffers: the pool must have drained before the interpreter frees them,
        # also when an exception unwinds past the owner or the process exits without close()
        import atexit
        atexit.register(self.close)

    def close(self):
        if self.h:
            self.lib.qpgpu_pool_destroy(self.h)      # drains the queue first
            self.h = None
            self._keep.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def proof_size(self):
        return self.lib.qpgpu_pool_proof_size(self.h)

    def set_witness_check(self, on=True):
        rc = self.lib.qpgpu_pool_set_witness_check(self.h, 1 if on else 0)
        if rc != 0:
            raise QpGpuError(rc, self.lib.qpgpu_pool_last_error(self.h).decode())

    def submit(self, d_wires, public_inputs, out=None):
        """Queue one proof of a device-resident witness; returns a ticket for wait()."""
        p = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        if out is None:
            out = np.empty(self.proof_size(), dtype=np.uint8)
        t = ctypes.c_uint64()
        rc = self.lib.qpgpu_pool_submit(self.h, _ptr(d_wires), p.ctypes.data, out.ctypes.data, out.size, ctypes.byref(t))
        if rc != 0:
            raise QpGpuError(rc, self.lib.qpgpu_pool_last_error(self.h).decode())
        self._keep[t.value] = (p, out, d_wires)
        return t.value

    def _submitted(self, rc, t, keep):
        if rc != 0:
            raise QpGpuError(rc, self.lib.qpgpu_pool_last_error(self.h).decode())
        self._keep[t.value] = keep
        return t.value

    def submit_on(self, device_index, d_wires, public_inputs, out=None):
        """A device-resident witness on the pool's device number `device_index` (only that device's workers take it)."""
        p = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        out = np.empty(self.proof_size(), dtype=np.uint8) if out is None else out
        t = ctypes.c_uint64()
        rc = self.lib.qpgpu_pool_submit_on(self.h, device_index, _ptr(d_wires), p.ctypes.data, out.ctypes.data, out.size, ctypes.byref(t))
        return self._submitted(rc, t, (p, out, d_wires))

    def submit_host(self, wires, public_inputs, out=None):
        """A full wire matrix in host memory (any worker of any device uploads and proves it)."""
        w = np.ascontiguousarray(wires, dtype=np.uint64); p = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        out = np.empty(self.proof_size(), dtype=np.uint8) if out is None else out
        t = ctypes.c_uint64()
        rc = self.lib.qpgpu_pool_submit_host(self.h, w.ctypes.data, p.ctypes.data, out.ctypes.data, out.size, ctypes.byref(t))
        return self._submitted(rc, t, (p, out, w))

    def set_partial_cells(self, cells, n_blinding=0):
        """n_blinding: the last n_blinding cells are the blinding wires of a zero-knowledge circuit, drawn on the device per proof."""
        cl = np.ascontiguousarray(cells, dtype=np.uint64)
        rc = self.lib.qpgpu_pool_set_partial_cells_blinded(self.h, cl.ctypes.data, cl.size, n_blinding)
        if rc != 0:
            raise QpGpuError(rc, self.lib.qpgpu_pool_last_error(self.h).decode())
        self._ncells = cl.size - n_blinding

    def submit_partial(self, values, public_inputs, out=None):
        """A PartialWitness over the pool's cell list: stage s1 on the device, then the proof. public_inputs=None: the proof carries
        the public inputs its witness holds (circuits that compute them)."""
        v = np.ascontiguousarray(values, dtype=np.uint64)
        p = None if public_inputs is None else np.ascontiguousarray(public_inputs, dtype=np.uint64)
        assert v.size == self._ncells
        out = np.empty(self.proof_size(), dtype=np.uint8) if out is None else out
        t = ctypes.c_uint64()
        rc = self.lib.qpgpu_pool_submit_partial(self.h, v.ctypes.data, None if p is None else p.ctypes.data, out.ctypes.data, out.size, ctypes.byref(t))
        return self._submitted(rc, t, (p, out, None))

    def scrub(self):
        """Every worker, after the job it is in, overwrites its circuit workspace, resident witnesses and partial-witness buffers."""
        rc = self.lib.qpgpu_pool_scrub(self.h)
        if rc != 0:
            raise QpGpuError(rc, self.lib.qpgpu_pool_last_error(self.h).decode())

    def residue_scan(self, needles, regions=None, cap=16):
        """QpGpu.residue_scan on every worker's context, totals summed: (hits, first_hits, bytes_scanned)."""
        rc, hits, first, nbytes = _residue_call(self.lib.qpgpu_pool_residue_scan, self.h, needles, regions, cap)
        if rc != 0:
            raise QpGpuError(rc, self.lib.qpgpu_pool_last_error(self.h).decode())
        return hits, first, nbytes

    def wait(self, ticket, copy=True):
        """The proof of a ticket (bytes); copy=False: only its length — the bytes are in the `out` buffer given to submit()."""
        ln = ctypes.c_size_t()
        rc = self.lib.qpgpu_pool_wait(self.h, ticket, ctypes.byref(ln))
        p, out, _ = self._keep.pop(ticket, (None, None, None))
        if rc != 0:
            raise QpGpuError(rc, self.lib.qpgpu_pool_last_error(self.h).decode())
        return out[:ln.value].tobytes() if copy else ln.value


class _ResidueAudit:
    def __init__(self, gpu, needles, cap):
        self.gpu, self.cap = gpu, cap
        self.needles = np.ascontiguousarray(needles, dtype=np.uint64)
        self.hits = self.buffers_released = None
        self.first_hits = []

    def __enter__(self):
        self.gpu._check(self.gpu.lib.qpgpu_ctx_residue_audit_begin(self.gpu.ctx, self.needles.ctypes.data, self.needles.size))
        return self

    def __exit__(self, *a):
        hits, released = ctypes.c_uint64(), ctypes.c_uint64()
        first = _blank_hits(self.cap)
        self.gpu._check(self.gpu.lib.qpgpu_ctx_residue_audit_end(self.gpu.ctx, ctypes.byref(hits), first, self.cap, ctypes.byref(released)))
        self.hits, self.buffers_released = hits.value, released.value
        self.first_hits = _written_hits(first, self.cap)


class _Stage3:
    """mixin: stage s3 wrappers"""

    def poseidon_permute(self, states):
        st = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 12)
        d = self.to_device(st)
        self._check(self.lib.qpgpu_poseidon_permute_dev(self.ctx, d.ptr, st.shape[0]))
        out = d.download().reshape(-1, 12)
        d.free()
        return out

    def poseidon2_hash_pad10(self, preimages, params=None):
        """The fork's application hash on the device (qpgpu_poseidon2_hash_pad10_dev): preimages [count, len] -> [count, 4].
        params None = qp-poseidon-core's pinned set; otherwise the 146-word block."""
        pre = np.ascontiguousarray(preimages, dtype=np.uint64)
        pre = pre.reshape(1, -1) if pre.ndim == 1 else pre
        count, ln = pre.shape
        d_in = self.to_device(pre) if pre.size else self.alloc(8)
        d_out = self.alloc(max(count, 1) * 32)
        try:
            if params is None:
                self._check(self.lib.qpgpu_poseidon2_hash_pad10_dev(self.ctx, None, 0, d_in.ptr, ln, count, d_out.ptr))
            else:
                blk = np.ascontiguousarray(params, dtype=np.uint64)
                self._check(self.lib.qpgpu_poseidon2_hash_pad10_dev(self.ctx, blk.ctypes.data, blk.size, d_in.ptr, ln, count, d_out.ptr))
            self.sync()
            return d_out.download()[:count * 4].reshape(count, 4).copy()
        finally:
            d_in.free(); d_out.free()

    def merkle_digest_count(self, log_leaves, cap_height):
        return self.lib.qpgpu_merkle_digest_count(log_leaves, cap_height)

    def merkle_build_dev(self, d_cols, col_stride, n_cols, log_leaves, cap_height, d_digests):
        cap = np.empty((1 << cap_height, 4), dtype=np.uint64)
        self._check(self.lib.qpgpu_merkle_build_dev(self.ctx, _ptr(d_cols), col_stride, n_cols, log_leaves,
                                                    cap_height, _ptr(d_digests), cap.ctypes.data))
        return cap

    def merkle_build_rows_dev(self, d_rows, width, log_leaves, cap_height, d_digests):
        cap = np.empty((1 << cap_height, 4), dtype=np.uint64)
        self._check(self.lib.qpgpu_merkle_build_rows_dev(self.ctx, _ptr(d_rows), width, log_leaves, cap_height,
                                                         _ptr(d_digests), cap.ctypes.data))
        return cap


class QpGpu(_Stage3):
    """One context = one GPU + one HIP stream."""

    def __init__(self, device=0, stream=None, hasher=None):
        """hasher: None = the process default; "poseidon"; or the Poseidon2 block (rc_ext, rc_int, diag_m1, m4)."""
        self.lib = load_library()
        ctx = ctypes.c_void_p()
        rc = self.lib.qpgpu_ctx_create(device, ctypes.byref(ctx))
        if rc != 0:
            raise QpGpuError(rc, "qpgpu_ctx_create failed (no gfx950 device visible?)")
        self.ctx = ctx
        if hasher is not None:
            if isinstance(hasher, str):
                self._check(self.lib.qpgpu_ctx_set_hasher(self.ctx, 0, None, 0))
            else:
                flat = _p2_block(*hasher)
                self._check(self.lib.qpgpu_ctx_set_hasher(self.ctx, 1, flat.ctypes.data, flat.size))
        if stream is not None:
            self._check(self.lib.qpgpu_ctx_set_stream(self.ctx, ctypes.c_void_p(stream)))

    def close(self):
        if self.ctx:
            self.lib.qpgpu_ctx_destroy(self.ctx)
            self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise QpGpuError(rc, self.lib.qpgpu_last_error(self.ctx).decode())

    def last_error(self):
        return self.lib.qpgpu_last_error(self.ctx).decode()

    def sync(self):
        self._check(self.lib.qpgpu_sync(self.ctx))

    def commit_sharded(self, ctxs, polys, **kw):
        """PolyOracle.commit_sharded with this context as the home context: ctxs is the full list of QpGpu objects, self first."""
        assert ctxs and ctxs[0] is self, "the home context comes first"
        return PolyOracle.commit_sharded(ctxs, polys, **kw)

    def pci_bus_id(self):
        """"dddd:bb:dd.f" of the context's device (the key of its sysfs directory)."""
        buf = ctypes.create_string_buffer(16)
        self._check(self.lib.qpgpu_ctx_pci_bus_id(self.ctx, buf, 16))
        return buf.value.decode()

    def profile(self, on=True):
        self._check(self.lib.qpgpu_profile_enable(self.ctx, 1 if on else 0))

    def profile_read(self, kernel):
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        self._check(self.lib.qpgpu_profile_read(self.ctx, kernel.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def residue_scan(self, needles, regions=None, cap=16):
        """Looks for the 64-bit needle words in every device / pinned buffer the library allocated for this context (a test
        facility). regions: None (every region that can hold witness-derived words), region names, or a bit mask. Returns
        (hits, first_hits, bytes_scanned); first_hits: up to `cap` dicts (word, region, pinned, offset_words, alloc_bytes)."""
        rc, hits, first, nbytes = _residue_call(self.lib.qpgpu_ctx_residue_scan, self.ctx, needles, regions, cap)
        self._check(rc)
        return hits, first, nbytes

    def residue_audit(self, needles, cap=16):
        """Context manager: every tracked buffer the library frees inside the block is scanned for the needles right before the
        free. The object it yields has hits, first_hits and buffers_released once the block has ended."""
        return _ResidueAudit(self, needles, cap)

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        return DeviceBuffer(self, arr.nbytes).upload(arr)

    def field_probe(self, op, a, b=None, param=0):
        """qpgpu_field_probe on the device: one primitive of the device field code, one thread per index (test hook)."""
        rc, out = _field_probe(self.ctx, op, a, b, param, True)
        self._check(rc)
        return out

    # ---- stage s2 ----
    def ntt_host(self, data, log_n, inverse=False, coset_shift=0, bitrev=False):
        """plonky2 fft / ifft / coset_fft on a host array [batch, 2^log_n]; returns a new array."""
        a = np.array(data, dtype=np.uint64, copy=True).reshape(-1, 1 << log_n)
        flags = (NTT_INVERSE if inverse else 0) | (NTT_OUT_BITREV if bitrev else 0)
        self._check(self.lib.qpgpu_ntt_batch(self.ctx, a.ctypes.data, log_n, a.shape[0], flags, coset_shift))
        return a

    def ntt_dev(self, d_in, d_out, log_n, batch, inverse=False, coset_shift=0, bitrev=False):
        flags = (NTT_INVERSE if inverse else 0) | (NTT_OUT_BITREV if bitrev else 0)
        self._check(self.lib.qpgpu_ntt_batch_dev(self.ctx, _ptr(d_in), _ptr(d_out), log_n, batch, flags, coset_shift))

    def lde_dev(self, d_coeffs, d_out, log_n, rate_bits, batch, coset_shift=MULT_GEN, bitrev=False):
        flags = NTT_OUT_BITREV if bitrev else 0
        self._check(self.lib.qpgpu_lde_batch_dev(self.ctx, _ptr(d_coeffs), _ptr(d_out), log_n, rate_bits, batch, flags, coset_shift))


def _ptr(x):
    if isinstance(x, DeviceBuffer):
        return x.ptr
    if hasattr(x, "data_ptr"):  # torch tensor living in HBM
        return x.data_ptr()
    return int(x)
