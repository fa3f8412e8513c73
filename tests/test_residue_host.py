"""The secret residue audit (include/qpgpu.h, csrc/residue.hpp), the part that needs no device: the registry's bookkeeping as a
stand-alone program over host memory under AddressSanitizer and UndefinedBehaviorSanitizer (tests/native/residue_registry_main.cpp
compiled together with csrc/residue.cpp, which has no HIP call in it), the region names, the hit structure's layout and the new
exports' refusal of NULL handles. The scan itself and the holes it found are tested on the device by tests/test_residue_gpu.py.
This is the counterpart of the reference's allocator bookkeeping in wormhole/circuit/tests/heap_zeroization.rs."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REGIONS = ["circuit-setup", "circuit-workspace", "witness-plan", "partial-witness", "ctx-scratch", "ctx-pinned", "oracle", "stage-plan",
           "fri-session", "pool-witness", "verify-staging", "zk-tree", "tables"]


def test_registry_program_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "qp-zk-circuits_amd", "csrc")
    exe = str(tmp_path / "residue_registry")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I", csrc,
                           os.path.join(ROOT, "tests", "native", "residue_registry_main.cpp"), os.path.join(csrc, "residue.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.split("\n")[:-1] == ["names ok", "masks ok", "cap ok", "refusals ok", "audit ok", "backend ok", "residue registry: ok"]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_region_names_and_hit_layout(pkg):
    lib = pkg.load_library()
    for i, name in enumerate(REGIONS):
        assert lib.qpgpu_residue_region_name(i) == name.encode(), i
    assert lib.qpgpu_residue_region_name(len(REGIONS)) is None and lib.qpgpu_residue_region_name(0xFFFFFFFF) is None
    assert pkg.binding.residue_regions() == REGIONS
    # typedef struct { uint64_t word; uint32_t region; uint32_t pinned; uint64_t offset_words; uint64_t alloc_bytes; } qpgpu_residue_hit;
    H = pkg.binding.ResidueHit
    assert ctypes.sizeof(H) == 32
    assert [(n, getattr(H, n).offset, getattr(H, n).size) for n, _ in H._fields_] == [
        ("word", 0, 8), ("region", 8, 4), ("pinned", 12, 4), ("offset_words", 16, 8), ("alloc_bytes", 24, 8)]
    assert pkg.binding.RESIDUE_MAX_NEEDLES == 16
    hdr = open(os.path.join(ROOT, "include", "qpgpu.h")).read()
    assert "#define QPGPU_RESIDUE_MAX_NEEDLES 16" in hdr
    assert "typedef struct { uint64_t word; uint32_t region; uint32_t pinned; uint64_t offset_words; uint64_t alloc_bytes; } qpgpu_residue_hit;" in hdr
    assert pkg.binding._residue_mask(None) == 0 and pkg.binding._residue_mask(["oracle", "ctx-pinned"]) == (1 << 6) | (1 << 5)


def test_new_exports_refuse_null_handles(pkg):
    lib = pkg.load_library()
    needles = (ctypes.c_uint64 * 2)(0xDEADBEEFCAFEF00D, 0x0123456789ABCDEF)
    hits, nbytes = ctypes.c_uint64(77), ctypes.c_uint64(77)
    first = (pkg.binding.ResidueHit * 2)()
    assert lib.qpgpu_ctx_residue_scan(None, needles, 2, 0, ctypes.byref(hits), first, 2, ctypes.byref(nbytes)) == -1
    assert lib.qpgpu_ctx_residue_scan(None, None, 0, 0, None, None, 0, None) == -1
    assert lib.qpgpu_ctx_residue_audit_begin(None, needles, 2) == -1 and lib.qpgpu_ctx_residue_audit_begin(None, None, 0) == -1
    assert lib.qpgpu_ctx_residue_audit_end(None, ctypes.byref(hits), first, 2, ctypes.byref(nbytes)) == -1
    assert lib.qpgpu_pool_scrub(None) == -1
    assert lib.qpgpu_pool_residue_scan(None, needles, 2, 0, ctypes.byref(hits), first, 2, ctypes.byref(nbytes)) == -1
    assert hits.value == 77 and nbytes.value == 77 and list(needles) == [0xDEADBEEFCAFEF00D, 0x0123456789ABCDEF]


def test_python_surface(pkg):
    for name in ("residue_scan", "residue_audit"):
        assert callable(getattr(pkg.QpGpu, name))
    for name in ("scrub", "residue_scan"):
        assert callable(getattr(pkg.ProvingPool, name))
    assert callable(pkg.leaf.LeafProver.scrub)
    names = pkg.binding.exported_symbols()
    for n in ("qpgpu_ctx_residue_scan", "qpgpu_residue_region_name", "qpgpu_ctx_residue_audit_begin", "qpgpu_ctx_residue_audit_end",
              "qpgpu_pool_scrub", "qpgpu_pool_residue_scan"):
        assert n in names and hasattr(pkg.load_library(), n), n
