"""CPU: the shape of the f32 lane kernel's tile body in the compiled gfx950 code (hipcc cross-compiles here).

On gfx9 parts vmcnt counts stores as well as loads, so a wait for a load issued after a store also waits for that store. The
tile body therefore issues every load of the lane's four pixels, waits once, and then stores back to back: for
fuse_lane_kernel<u8, pose>'s whole-tile path, every vector-memory load of the tile comes before its first
global_store_dwordx3 and no vmcnt wait sits between its stores. Scratch stays 0 and occupancy 8."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

from helpers import ROOT

spec = importlib.util.spec_from_file_location("isa_barrier_check", os.path.join(ROOT, "tools", "isa_barrier_check.py"))
chk = importlib.util.module_from_spec(spec)
spec.loader.exec_module(chk)

KERNEL = "fuse_lane_kernelIhLb1ELb0E"      # fuse_lane_kernel<unsigned char, true (pose), false (element loads)>
VMEM_LOAD = re.compile(r"^\s*(global_load|buffer_load|flat_load)")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if shutil.which(chk.HIPCC) is None and not os.path.exists(chk.HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "r3d_fuse.s")
    r = subprocess.run([chk.HIPCC] + chk.FLAGS + [os.path.join(chk.CSRC, "r3d_fuse.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


def kernel(asm):
    names = [n for n in chk.functions(asm) if KERNEL in n]
    assert len(names) == 1, names
    return names[0], [l.split(";")[0].rstrip() for l in chk.functions(asm)[names[0]]]


def test_whole_tile_loads_first_then_stores_without_waits(asm):
    _, body = kernel(asm)
    stores = [i for i, l in enumerate(body) if l.strip().startswith("global_store_dwordx3")]
    assert len(stores) >= 4, "no x3 stores found"
    s0, s3 = stores[0], stores[3]
    # the whole-tile path: the first four x3 stores, in one straight run of code
    run = body[s0:s3 + 1]
    assert not any(l.startswith(".LBB") or l.strip().startswith("s_cbranch") for l in run), "\n".join(run)
    assert not any(l.strip().startswith("s_waitcnt") and "vmcnt" in l for l in run), "\n".join(run)
    assert not any(VMEM_LOAD.match(l) for l in run), "\n".join(run)
    # the tile loop's loads: from the loop header (the last label in front of the tile's first load) up to the first store
    first_load = next(i for i, l in enumerate(body) if VMEM_LOAD.match(l))
    header = max(i for i in range(first_load) if body[i].startswith(".LBB"))
    loads = [i for i in range(header, s0) if VMEM_LOAD.match(body[i])]
    assert len(loads) == 12, len(loads)                 # 4 depth bytes + 4 u + 4 v per lane
    waits = [i for i in range(loads[-1], s0) if body[i].strip().startswith("s_waitcnt") and "vmcnt" in body[i]]
    assert len(waits) == 1, [body[i] for i in waits]   # one wait, after the last load
    # nothing after the last store of the run goes back to memory before the loop's back edge
    after = body[s3 + 1:]
    nxt = next((i for i, l in enumerate(after) if l.startswith(".LBB")), len(after))
    assert not any(VMEM_LOAD.match(l) for l in after[:nxt])


def test_no_scratch_and_occupancy_8(asm):
    name, _ = kernel(asm)
    m = re.search(r"^" + re.escape(name) + r":.*?; ScratchSize: (\d+).*?; Occupancy: (\d+)", asm, re.S | re.M)
    assert m, "no resource comment for " + name
    assert int(m.group(1)) == 0 and int(m.group(2)) == 8, m.groups()
