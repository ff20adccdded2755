"""azg_pv_score_outputs' argument checks (include/azg_pv.h), without a GPU: they run before
any device call, so a bad call returns nonzero with azg_pv_last_error() text and never
touches its pointers (the dummy addresses below are never dereferenced)."""
import re

import pytest

import _native
from conftest import REPO

P = 0x1000   # a non-null stand-in for a device pointer


def _call(lib, logits=P, values=P, pis=P, zs=P, batch=16, per_board=P, sums=P):
    return lib.azg_pv_score_outputs(logits, values, pis, zs, batch, per_board, sums, None)


@pytest.mark.parametrize("arg", ["logits", "values", "pis", "zs", "per_board"])
def test_score_outputs_rejects_a_null_argument(arg):
    lib = _native.load_library()
    assert _call(lib, **{arg: None}) != 0
    msg = lib.azg_pv_last_error()
    assert msg and b"azg_pv_score_outputs" in msg and arg.encode() in msg


@pytest.mark.parametrize("batch", [0, -1])
def test_score_outputs_rejects_an_empty_batch(batch):
    lib = _native.load_library()
    assert _call(lib, batch=batch) != 0
    assert _call(lib, batch=batch, sums=None) != 0
    msg = lib.azg_pv_last_error()
    assert msg and b"azg_pv_score_outputs" in msg and b"batch" in msg


def test_exported_and_abi_version_unchanged():
    lib = _native.load_library()
    assert "azg_pv_score_outputs" in _native.EXPORTS and hasattr(lib, "azg_pv_score_outputs")
    assert lib.azg_pv_abi_version() == 3 == _native.ABI_VERSION


def test_header_field_enum_equals_the_python_names():
    from engine import SCORE_FIELDS
    txt = open(f"{REPO}/include/azg_pv.h").read()
    fields = {name: int(num) for name, num in re.findall(r"AZG_PV_SCORE_([A-Z0-9_]+)\s*=\s*(\d+)", txt)}
    assert fields.pop("FIELDS") == 8 == len(SCORE_FIELDS)
    assert fields == {n.upper(): i for i, n in enumerate(SCORE_FIELDS)}
