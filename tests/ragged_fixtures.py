"""The ragged-update fixtures (tests/golden/make_golden_ragged.py: one reference PPO.update() each at obs 77, hidden
[320, 260, 64] and at obs 19, hidden [64, 64]), stored as three files of one key group each; wide_fixtures puts such
files back together and runs the update that update_fixtures.build_update / check_update bracket."""

import json
import os

from conftest import GOLDEN
from wide_fixtures import Arrays, run_update  # noqa: F401

CASES = ("ragged_wide", "ragged_narrow")


def load(name):
    with open(os.path.join(GOLDEN, "golden_ragged.json")) as f:
        meta = json.load(f)[name]
    return Arrays(meta["files"]), meta
