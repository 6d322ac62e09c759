"""Recorder of tests/golden/sums_bits.json: the raw words of the fp64 sums (18 pair sums, 29 point-to-plane sums, the RANSAC
refit's 10) and of the ICP states that the estimation loops produce for the cases of tests/sums_bits_cases.py.

Run ONCE, on the GPU, with the library built from the commit whose arithmetic is to be pinned:

    python tests/golden/make_sums_bits.py <commit hash> [output path]

tests/test_gpu_sums_bits.py then demands these very words from every later build; it never writes the file.  A case that is
trivial (few pairs, a degenerate step, a state whose status is not 0) is refused here, so that it cannot become the golden."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

try:
    import torch  # noqa: F401  (first, as in tests/conftest.py: one HIP runtime per process)
except ImportError:
    pass

import sums_bits_cases as SC  # noqa: E402
from helpers import r3d  # noqa: E402


def check(name, facts):
    n = facts["n"]
    # trim_q = 0.5 with gate_scale = 1 keeps half of the admissible pairs by design, so that one plane case cannot reach half the
    # source: it takes the bound of test_29_sums_match_oracle_and_are_repeatable (3000 of 12288) instead
    floor = 3000 if name == "plane_0.5_1_-1" else n / 2
    for pairs in facts["pairs"]:
        assert pairs > floor, (name, "too few pairs", pairs, floor)
    for st in facts.get("states", []):
        assert st["status"] == 0.0 and st["iterations"] == 3.0 and st["pairs"] > floor, (name, "degenerate state", st)
    assert facts.get("finite", True), (name, "no plane")


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "sums_bits.json")
    ctx = r3d().Context(0)
    cases = {}
    for name in SC.CASES:
        bits, facts = SC.run(name, ctx)
        check(name, facts)
        cases[name] = bits
        print(name, facts, flush=True)
    ctx.close()
    with open(out, "w") as f:
        json.dump({"recorded_at_commit": commit, "compute_units": SC.compute_units(), "generator": "tests/golden/make_sums_bits.py",
                   "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
