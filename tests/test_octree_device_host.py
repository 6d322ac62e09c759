"""CPU: what the device octree serialiser offers without a device -- exported symbols, the .bt header, argument errors, the
compiled kernels' register budget -- and the one-pass formulation (tests/octree_ref.py) pinned to oracle/octomap_ref."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import octree_ref
from helpers import PKG, ROOT
from oracle import octomap_ref as OM

NEW = ("r3d_octree_records_device", "r3d_octree_bt_header", "r3d_voxelset_format_bt", "r3d_voxelset_write_bt")
INVALID = -1


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def lib(L):
    return L.load()


def test_symbols_exported_and_bound(L, lib):
    header = open(os.path.join(ROOT, "include", "r3d.h")).read()
    for name in NEW:
        assert name in L.SIGNATURES and hasattr(lib, name) and re.search(r"\bint %s\(" % name, header)
    assert lib.r3d_version() == 200


def _header(lib, nodes, res, cap=256):
    buf, n = C.create_string_buffer(max(cap, 1)), C.c_size_t()
    rc = lib.r3d_octree_bt_header(nodes, res, buf, cap, C.byref(n))
    return rc, buf.raw[:n.value]


@pytest.mark.parametrize("size", [0, 1, 201_700_000])
@pytest.mark.parametrize("res", [0.1, 0.25, 1e-3, 2])
def test_header_equals_the_oracles(L, lib, size, res):
    want = OM.write_bt_bytes(np.zeros(0, np.uint64), res)[0].replace(b"size 0\n", b"size %d\n" % size)
    assert want.endswith(b"data\n") and (b"size %d\n" % size) in want
    rc, got = _header(lib, size, float(res))
    assert rc == 0 and got == want
    n = C.c_size_t()
    assert lib.r3d_octree_bt_header(size, float(res), None, 0, C.byref(n)) == 0 and n.value == len(want)   # length only
    rc, _ = _header(lib, size, float(res), cap=len(want))                                                  # exact fit
    assert rc == 0
    # the host serialiser takes its header from the same function
    V = importlib.import_module(PKG + ".voxelmap")
    data, nodes = V.format_bt(np.array([7 << 45], np.uint64), res)
    assert data.startswith(_header(lib, nodes, float(res))[1])


def test_argument_errors_need_no_device(L, lib):
    n, n64, m64 = C.c_size_t(), C.c_int64(), C.c_int64()
    buf = C.create_string_buffer(256)
    assert lib.r3d_octree_bt_header(1, 0.0, buf, 256, C.byref(n)) == INVALID
    assert lib.r3d_octree_bt_header(1, -0.1, buf, 256, C.byref(n)) == INVALID
    assert lib.r3d_octree_bt_header(1, float("nan"), buf, 256, C.byref(n)) == INVALID
    assert lib.r3d_octree_bt_header(-1, 0.1, buf, 256, C.byref(n)) == INVALID
    assert lib.r3d_octree_bt_header(1, 0.1, buf, 256, None) == INVALID
    before = buf.raw
    assert lib.r3d_octree_bt_header(17, 0.1, buf, 20, C.byref(n)) == INVALID and "too small" in L.last_error()
    assert buf.raw == before
    assert lib.r3d_octree_records_device(None, None, 5, None, 0, C.byref(n64), C.byref(m64)) == INVALID
    assert lib.r3d_octree_records_device(None, None, -1, None, 0, C.byref(n64), C.byref(m64)) == INVALID
    assert lib.r3d_voxelset_format_bt(None, None, 0, C.byref(n), C.byref(n64)) == INVALID
    assert lib.r3d_voxelset_write_bt(None, b"/nonexistent/x.bt", C.byref(n64)) == INVALID
    assert not os.path.exists("/nonexistent/x.bt")


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_no_octree_kernel_uses_scratch(tmp_path):
    """tools/isa_stats.py on the gfx950 listing of csrc/r3d_octree.hip: four kernels, no private segment, no spills."""
    src, out = os.path.join(ROOT, PKG, "csrc", "r3d_octree.hip"), str(tmp_path / "octree.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                    "--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True)
    r = subprocess.run(["python3", os.path.join(ROOT, "tools", "isa_stats.py"), out, "octree_"], check=True, capture_output=True, text=True)
    kernels = re.findall(r"^(\S*octree_(\w+?)_kernel\S*) instrs", r.stdout, re.M)
    assert sorted(k for _, k in kernels) == ["count", "link", "own", "scan"], r.stdout
    assert "scratch_" not in r.stdout and "buffer_" not in r.stdout
    text = open(out).read()
    assert len(re.findall(r"\.amdhsa_private_segment_fixed_size 0\n", text)) == 4 == text.count(".amdhsa_private_segment_fixed_size")
    assert set(re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)) == {"0"}
    assert set(re.findall(r"\.sgpr_spill_count:\s+(\d+)", text)) == {"0"}
    assert "global_atomic_or " in text and "global_atomic_or v" in text   # the link's OR, and its result is not asked for
    assert not re.search(r"global_atomic_or v\d+, v\d+, v\d+, s\[\d+:\d+\].*\bsc0\b", text)


def _cases():
    rng = np.random.default_rng(0)
    yield [5]
    yield [0]
    yield np.arange(8)
    yield np.arange(64) + 64 * 7
    yield np.arange(512)
    yield list(range(8, 16)) + [17, 2 ** 47 + 3]
    for s in range(6):
        yield OM.occupied_set(rng.normal(0, [0.3, 2, 6, .5, 1, 3][s], (3000, 3)))[0]
    k = np.stack(np.meshgrid(*[np.arange(32760, 32790)] * 3, indexing="ij"), -1).reshape(-1, 3)
    yield OM.morton(k)
    yield OM.morton(k[rng.random(len(k)) < 0.97])
    a = np.arange(4096) + 4096 * 5
    for cs in (a, a[1:], np.delete(a, 2000), a[:-1], np.arange(8192) + 4096 * 6, np.arange(4096) + 100, [0, 2 ** 48 - 1],
               [3, 3 + (1 << 45)], [8, 9]):
        yield cs


def test_one_pass_formulation_equals_the_oracle():
    n_cases = 0
    for cs in _cases():
        codes = np.unique(np.asarray(cs, np.uint64))
        ref, ref_nodes = OM.write_bt_bytes(codes, 0.1)
        body, nodes = octree_ref.bt_body(codes)
        assert ref.endswith(b"data\n" + body) and nodes == ref_nodes
        n_cases += 1
    assert n_cases == 23 and octree_ref.bt_body(np.zeros(0, np.uint64)) == (b"", 0)
