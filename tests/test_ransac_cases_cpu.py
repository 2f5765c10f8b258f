"""CPU: the named cases of both RANSAC terms did not move -- every table entry's generator-only tensors and the integer decisions
of its float64 composition against the checksums recorded before the cases modules shared tests/ransac_cases.py."""
import json
import os

from tests import ransac_cases as RC


def test_every_named_case_carries_the_recorded_checksums(golden_dir):
    with open(os.path.join(golden_dir, "ransac_case_checksums.json")) as fh:
        want = json.load(fh)
    got = RC.checksums()
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], (name, {k: (got[name][k], v) for k, v in want[name].items() if got[name][k] != v})
