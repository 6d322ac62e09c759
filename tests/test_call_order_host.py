"""No device: every csrc/*.hip file that claims a workspace of the context (a call to r3d_scratch) is named in the
catalogue's COVERS, so an entry point added later fails here until it has a case in tests/call_order_cases.py."""
import glob
import os
import re

import call_order_cases as CAT
from helpers import PKG, ROOT

CSRC = os.path.join(ROOT, PKG, "csrc")


def test_every_file_that_takes_a_scratch_slot_is_covered():
    takes = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hip"))
                   if re.search(r"\br3d_scratch\(", open(p).read()))
    assert len(takes) >= 24, takes   # (25 while r3d_tsdf_color.hip had a host-slab uploader of its own: r3d_tsdf.hip's serves both now)
    covered = {f for files in CAT.COVERS.values() for f in files}
    assert not [f for f in takes if f not in covered], "files with r3d_scratch( and no case in COVERS"


def test_covers_names_real_files_and_real_cases():
    for case, files in CAT.COVERS.items():
        assert case in CAT.CASES or case == "not_covered_multi_device", case
        for f in files:
            assert os.path.exists(os.path.join(CSRC, f)), (case, f)
    assert set(CAT.CASES) <= set(CAT.COVERS)
    assert "not_covered_multi_device" not in CAT.CASES
