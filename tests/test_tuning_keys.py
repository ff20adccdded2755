"""The tuning keys of azg_pv_set_tuning (csrc/pv_tuning.hip), without a GPU: every key's
accepted values, default and return values against the recorded table of the product
library (tests/golden/tuning_keys.json), and the key names of the header against
_native.TUNE."""
import json
import os
import re
import subprocess
import sys

import pytest

from conftest import GOLDEN, REPO

import _native

HEADER = os.path.join(REPO, "include", "azg_pv.h")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "tuning_keys.json")) as f:
        return json.load(f)


def test_every_key_returns_the_recorded_sequence(golden):
    # a fresh child process: an empty autotune cache, every variable at its default, and no
    # other test sees the keys it changes; it loads the library and touches no GPU
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_tuning.py"), "--print"], env=env,
                         check=True, capture_output=True, text=True, timeout=300).stdout
    got = json.loads(out)
    assert got["values"] == golden["values"]
    assert list(got["returns"]) == list(golden["returns"])
    for key, seq in golden["returns"].items():
        assert got["returns"][key] == seq, f"key {key}"


def test_header_enum_equals_native_names():
    txt = open(HEADER).read()
    body = re.search(r"enum azg_pv_tuning_key \{(.*?)\n\};", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    header = {name: int(num) for name, num in re.findall(r"AZG_PV_TUNE_([A-Z0-9_]+)\s*=\s*(\d+)", body)}
    assert header == {m.name: m.value for m in _native.TUNE}


def test_every_accepted_key_has_a_name(golden):
    accepted = {int(k) for k, seq in golden["returns"].items() if any(r != -1 for r in seq)}
    assert accepted <= {m.value for m in _native.TUNE}
