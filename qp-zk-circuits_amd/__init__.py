"""qp-zk-circuits_amd — MI355X (gfx950) backend for the qp-wormhole proving hot path.

The product is libqpgpu.so (hand-written HIP kernels behind the C ABI of include/qpgpu.h).
This Python package is only the ctypes harness used by tests/ and bench.py; it never falls back
to a CPU implementation: if the shared library or a GPU is missing, calls raise.

The directory name carries a hyphen (it mirrors the reference repository's name), so it is
imported through `__graft_entry__.load_package()` under the module name `qp_zk_circuits_amd`.
"""
from .binding import poseidon_constants, synth_circuit, Circuit, QpGpu, QpGpuError, lib_path, load_library, P, MULT_GEN  # noqa: F401
from .binding import StagePlan, stage_header_words  # noqa: F401
from .binding import WitnessFinding, format_finding, FINDING_GATE, FINDING_COPY  # noqa: F401
from .binding import FriSession, fri_grind  # noqa: F401
from .binding import FriVerifier  # noqa: F401
from .binding import fri_prove_batch, fri_grind_batch  # noqa: F401
from .binding import PolyOracle, Challenger, fri_prove, set_hasher_poseidon, set_hasher_poseidon2, ProvingPool  # noqa: F401
from .binding import pack_header, pack_public_input_cells, Verifier, poseidon2_qp_params, synth_p2_sites  # noqa: F401
from .binding import pack_p2_layout, pack_trailers, p2_site_cells, P2_NO_SWAP  # noqa: F401
from .binding import CircuitConfig, circuit_config, validate_circuit_config  # noqa: F401
from .binding import AggConfigArgs, agg_config_args, agg_config_validate, agg_config_build, parse_agg_config_flags  # noqa: F401
from .binding import FP, FP_OPS, field_probe_host, field_probe_shape  # noqa: F401
from . import sharding  # noqa: F401,E402
from . import aggregation  # noqa: F401,E402
from . import leaf  # noqa: F401,E402
from . import recursion  # noqa: F401,E402
