"""The C-ABI library builds for gfx950, loads, and exports every symbol include/storm_hip.h declares
(no compute calls: CPU suite)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "storm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(storm_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_and_exports_every_declared_symbol():
    from storm_amd.build import build
    path = build()
    lib = ctypes.CDLL(path)
    names = declared_symbols()
    assert len(names) >= 28
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    lib.storm_abi_version.restype = ctypes.c_int
    assert lib.storm_abi_version() == 2
    lib.storm_last_error.restype = ctypes.c_char_p
    assert lib.storm_last_error() is not None
    # the sizes the binding refuses a library by (storm_abi_struct_bytes), asked of the library directly
    from storm_amd import _lib
    lib.storm_abi_struct_bytes.restype, lib.storm_abi_struct_bytes.argtypes = ctypes.c_longlong, [ctypes.c_int]
    for which, cls in enumerate((_lib.ConvArgs, _lib.Op, _lib.ConvSeg, _lib.NcsnppConfig, _lib.NcsnppConfigEx)):
        assert lib.storm_abi_struct_bytes(which) == ctypes.sizeof(cls), cls.__name__
    assert lib.storm_abi_struct_bytes(5) == -1 and lib.storm_abi_struct_bytes(-1) == -1


def test_python_binding_covers_the_header():
    from storm_amd import _lib
    assert set(declared_symbols()) == set(_lib.EXPORTS)


# exported entry points that neither the product's Python nor a test calls (each with the reason it has no caller yet); a name that
# is not listed here must occur in storm_amd/ (outside the binding table itself) or in tests/
KNOWN_UNREACHED = [
    "storm_gn_apply_kernel_name",    # bench.py's per-op table only: the name of the kernel the GroupNorm-apply launcher picks
    "storm_ncsnpp_arena",            # bench.py's per-op table and tools/tune_dispatch.py only: the parameter arena behind a planned program
]


def test_every_export_is_reached_by_the_product_or_a_test():
    """An entry point that nothing calls is a kernel that nothing checks: every name of _lib.EXPORTS occurs (as a whole word) in the
    Python of storm_amd/ outside _lib.py or in a file under tests/.  The per-row-key forms are called as name + "_rs" by
    ops._noise_call: such a name counts as reached where its base name is handed to _noise_call."""
    import glob

    from storm_amd import _lib
    files = [f for f in glob.glob(os.path.join(ROOT, "storm_amd", "**", "*.py"), recursive=True) if os.path.basename(f) != "_lib.py"]
    for ext in ("py", "c", "h", "cpp"):
        files += glob.glob(os.path.join(ROOT, "tests", "**", "*." + ext), recursive=True)
    words = set()
    for f in files:
        text = open(f).read()
        if os.path.abspath(f) == os.path.abspath(__file__):
            text = re.sub(r"KNOWN_UNREACHED = \[.*?\n\]", "", text, flags=re.S)       # (the list itself is no caller)
        words |= set(re.findall(r"\bstorm_[a-z0-9_]+\b", text))
    ops_text = open(os.path.join(ROOT, "storm_amd", "ops.py")).read()
    noise_calls = set(re.findall(r"_noise_call\(\s*\"(storm_[a-z0-9_]+)\"", ops_text))
    assert 'name + "_rs"' in ops_text and noise_calls
    reached = words | {n + "_rs" for n in noise_calls}
    unreached = sorted(n for n in _lib.EXPORTS if n not in reached)
    assert unreached == sorted(KNOWN_UNREACHED), unreached
    assert not set(KNOWN_UNREACHED) & reached                          # (a listed name that has found a caller leaves the list)


def test_product_does_not_import_the_oracle():
    """the oracle is test infrastructure: nothing under storm_amd/ (or bench.py outside cpu_baseline) may use it"""
    import glob
    for f in glob.glob(os.path.join(ROOT, "storm_amd", "**", "*.py"), recursive=True):
        assert "oracle" not in open(f).read().replace("# oracle", ""), f
    bench = open(os.path.join(ROOT, "bench.py")).read()
    uses = [m.start() for m in re.finditer(r"from oracle|import oracle", bench)]
    base = bench.index("def cpu_baseline")
    nxt = bench.index("\ndef ", base + 1)
    assert uses and all(base < u < nxt for u in uses)


def _run_c_host(tmp_path, lib_path, compiler, extra, golden, ldflags=()):
    """compile tests/c/ncsnpp_host.c, hand it the reference's tiny4 golden input + the seeded state_dict as raw files, run it"""
    import subprocess

    import numpy as np
    import torch

    from oracle import ncsnpp_ref as NR
    g = golden["f2_tiny_nets"]
    cfg = NR.NCSNppConfig(nf=8, input_channels=4)
    sd = NR.seeded_state_dict(cfg, seed=7)
    d = str(tmp_path)
    for i, v in enumerate(sd.values()):
        v.detach().contiguous().numpy().astype(np.float32).tofile(os.path.join(d, f"w{i}.bin"))
    x = g["tiny4_x"]                                        # complex64 [2, 2, 32, 64]
    for j in range(2):
        np.ascontiguousarray(x[:, j]).tofile(os.path.join(d, f"x{j}.bin"))
    g["t"].astype(np.float32).tofile(os.path.join(d, "t.bin"))
    exe = os.path.join(d, "ncsnpp_host")
    libdir, libname = os.path.dirname(lib_path), os.path.basename(lib_path)[3:-3]
    cmd = [compiler] + extra + ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "ncsnpp_host.c"), "-o", exe,
                                "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir] + list(ldflags)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, d, "8", "4", "2", "32", "64", "0"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = np.fromfile(os.path.join(d, "out.bin"), dtype=np.complex64).reshape(2, 1, 32, 64)
    ref = g["tiny4_y"]
    err = float(np.linalg.norm(out - ref) / np.linalg.norm(ref))
    assert err < 1e-4, err
    return r.stdout


def test_c_host_runs_a_forward_through_the_whole_network_abi(tmp_path, golden):
    """A host written in C (no Python planning / packing / dispatch): storm_ncsnpp_tensor_info -> storm_ncsnpp_create ->
    storm_ncsnpp_workspace_bytes -> storm_ncsnpp_forward, linked against the host simulation of the kernels; its output
    equals the REFERENCE's forward of the tiny4 network (fixture F2, fp32 <= 1e-4)."""
    from tests.sim.build_sim import build
    out = _run_c_host(tmp_path, build(), "gcc", ["-std=c99", "-O1"], golden)
    assert "271 tensors" in out


import pytest  # noqa: E402

from tests.backend import dev  # noqa: E402,F401


def test_device_info(dev):
    """storm_device_info: the architecture name (truncated to the caller's buffer, always terminated), the compute units and the memory
    of the current device - torch's own numbers on the GPU, the host simulation's placeholders otherwise; every output is optional"""
    import torch

    from storm_amd import _lib
    lib = _lib.lib()
    name, n_cu, hbm = ctypes.create_string_buffer(b"\xff" * 64, 64), ctypes.c_int(-1), ctypes.c_size_t(1)
    _lib.check(lib.storm_device_info(name, 64, ctypes.byref(n_cu), ctypes.byref(hbm)), "storm_device_info")
    if dev.type == "cpu":
        assert (name.value, n_cu.value, hbm.value) == (b"host-sim", 0, 0)
    else:
        p = torch.cuda.get_device_properties(dev)
        assert name.value.decode() == p.gcnArchName and name.value.startswith(b"gfx950")
        assert n_cu.value == p.multi_processor_count > 0 and hbm.value == p.total_memory > 0
    short = ctypes.create_string_buffer(b"\xff" * 8, 8)
    _lib.check(lib.storm_device_info(short, 4, None, None), "storm_device_info")
    assert short.raw[:4] == name.value[:3] + b"\0" and short.raw[4:] == b"\xff" * 4
    _lib.check(lib.storm_device_info(None, 0, None, None), "storm_device_info")



@pytest.mark.gpu
def test_c_host_on_the_gpu(tmp_path, golden):
    """the same C host against libstorm_hip.so on the MI355X: plain g++ (-DUSE_HIP: device memory through the HIP runtime
    API, hipMalloc / hipMemcpy), no device code in the host program"""
    from storm_amd.build import build
    _run_c_host(tmp_path, build(), "g++", ["-x", "c++", "-DUSE_HIP", "-D__HIP_PLATFORM_AMD__", "-O1", "-I", "/opt/rocm/include"], golden,
                ldflags=["-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
