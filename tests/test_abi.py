"""The drop-in boundary: libgf_step.so loads without a GPU and exports every entry point include/gf_step.h declares,
with struct layouts identical to the ctypes binding and to the oracle's host twins."""
import ctypes
import os
import re

from genesis_forge_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "gf_step.h")).read()
    body = src[src.index("Entry points"):]
    return sorted(set(re.findall(r"\b(gf_[a-z_]+)\s*\(", body)))


def test_header_declares_all_phases():
    names = _declared()
    for fn in nat.PHASE_FUNCS:
        assert "gf_" + fn in names
    assert {"gf_run_ops", "gf_stats_clear", "gf_abi_version", "gf_sizeof", "gf_error_string", "gf_profile_begin", "gf_profile_end", "gf_set_option",
            "gf_event_create", "gf_event_synchronize", "gf_event_destroy", "gf_build_info"} <= set(names)


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(nat.lib_path())
    for name in _declared():
        assert hasattr(lib, name), f"{name} is declared in include/gf_step.h but not exported by libgf_step.so"
    nat.check_abi(lib, "gf_")
    lib.gf_error_string.restype = ctypes.c_char_p
    assert lib.gf_error_string(-3) == b"unknown opcode in term table"


def test_oracle_twin_layouts(oracle_lib_path):
    olib = ctypes.CDLL(oracle_lib_path)
    nat.check_abi(olib, "gfo_")
    for fn in nat.PHASE_FUNCS:
        assert hasattr(olib, "gfo_" + fn)


def test_product_package_never_touches_the_oracle():
    pkg = os.path.join(ROOT, "genesis-forge_amd")
    for base, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(base, f)).read()
                assert "libgf_oracle" not in text and "gfo_" not in text, f"{f} references the oracle"


def test_no_gpu_means_loud_failure():
    import pytest
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    b = nat.HipBackend()
    a = nat.GfRotateArgs()
    with pytest.raises(nat.GfError, match="no ROCm device"):
        b.call("entity_rotate", a)


def _kernel_resources(path):
    """{mangled kernel name: (scratch bytes per lane, VGPRs)} of the gfx950 code objects embedded in a built library: the clang
    offload bundles of its .hip_fatbin section, each code object's AMDGPU metadata note read with llvm-readelf."""
    import re
    import struct
    import subprocess
    import tempfile

    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    data = open(path, "rb").read()
    out, pos = {}, 0
    while True:
        i = data.find(magic, pos)
        if i < 0:
            break
        n, = struct.unpack_from("<Q", data, i + 24)
        off = i + 32
        for _ in range(n):
            o, sz, tsz = struct.unpack_from("<QQQ", data, off)
            triple = data[off + 24: off + 24 + tsz].decode()
            off += 24 + tsz
            if "gfx950" not in triple or not sz:
                continue
            with tempfile.NamedTemporaryFile(suffix=".co") as f:
                f.write(data[i + o: i + o + sz])
                f.flush()
                txt = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
            for m in re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)", txt, re.S):
                out[m.group(1)] = (int(m.group(2)), int(m.group(3)))
        pos = i + 24
    return out


READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def test_no_kernel_spills_to_scratch_and_the_fused_kernels_keep_their_occupancy():
    """A kernel of this library that touches private memory is a regression (a register block kept live across a run-time switch put
    the fused kernel's table interpreter there once: 10.9 -> 15.1 us at 65 536 envs before anything else noticed), and so is a fused
    kernel whose registers cost it a workgroup per CU: 512 VGPRs per SIMD lane, one wave of each resident workgroup per SIMD."""
    import pytest

    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf")
    res = _kernel_resources(nat.lib_path())
    assert len(res) >= 60, sorted(res)
    spilled = {k: v for k, v in res.items() if v[0]}
    assert not spilled, spilled

    def vgprs(fragment):
        hits = [v[1] for k, v in res.items() if fragment in k]
        assert len(hits) == 1, (fragment, hits)
        return hits[0]

    assert vgprs("post_ws_kernelINS_6InterpILi3ELb0EEE") <= 128      # 12-DOF interpreter: four workgroups per CU
    assert vgprs("post_ws_kernelINS_6InterpILi7ELb0EEE") <= 168      # 28-DOF interpreter: three
    assert vgprs("post_ws_kernelINS_23ProgGo2CommandDirectionE") <= 84   # the benchmark's program: six
    assert vgprs("post_ws_kernelINS_18ProgGo2GaitTrainerE") <= 100   # five


def test_the_fused_kernel_is_instantiated_for_exactly_the_programs_of_the_table():
    """post_ws_kernel<P> exists for the nine built-in programs and the 8 x 2 rows of the table interpreter, post_ws_kernel_tick<P> for
    the four programs that carry the tick prologue: a kernel more is ~1 150 source lines of build time and library size nobody launches
    (a helper that instantiates a tick variant per program adds twenty of them), a kernel less is a program the table cannot launch."""
    import pytest

    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf")
    builtin = ["23ProgGo2CommandDirection", "13ProgGo2Simple", "15ProgGo2Contacts", "19ProgGo2RoughTerrain", "20ProgBerkeleyHumanoid",
               "18ProgGo2GaitTrainer", "20ProgHumanoid28Stress", "23ProgGo2GaitTrainerFront", "21ProgGo2GaitTrainerObs"]
    interp = ["6InterpILi%dELb%dEE" % (dv, tail) for dv in range(1, 9) for tail in (0, 1)]
    tick = ["23ProgGo2CommandDirection", "13ProgGo2Simple", "6InterpILi3ELb0EE", "6InterpILi7ELb0EE"]
    want = {"_ZN2gf14post_ws_kernelINS_%sEEEvNS_10GfPostArgsE" % p for p in builtin + interp}
    want |= {"_ZN2gf19post_ws_kernel_tickINS_%sEEEvNS_10GfPostArgsE12GfActionArgs16GfSynthSceneArgsi" % p for p in tick}
    assert len(want) == 9 + 16 + 4
    have = {k for k in _kernel_resources(nat.lib_path()) if "post_ws_kernel" in k}
    assert have == want, (sorted(have - want), sorted(want - have))
