"""Golden table of azg_pv_set_tuning: what every key returns for a fixed sequence of
values, in a fresh process (empty autotune cache, every variable at its default).

The fixture pins the accepted values, the defaults and the unknown keys of the PRODUCT
library (built without AZG_AB_STUDIES).  It was recorded from the library of the commit
before the keys moved into the table of csrc/pv_tuning.hip; re-record it only from a
library whose key behaviour is the intended one, never to make a failing test pass:
  AZG_PV_LIB=/path/to/libazg_pv.so PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tuning.py
`--print` writes the table of the current library to stdout instead (tests/test_tuning_keys.py
runs it that way in a child process).  No GPU is touched.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "alphazero-gomoku_amd"))

KEYS = list(range(56)) + [999]
VALUES = [-2, -1, 0, 1, 2, 3, 4, 5, 8, 9, 10, 12, 13, 14, 16, 24, 64, 65, 100000]
PATH = os.path.join(HERE, "tuning_keys.json")


def probe() -> dict:
    import _native  # noqa: E402
    lib = _native.load_library()
    return {"values": VALUES, "returns": {str(k): [lib.azg_pv_set_tuning(k, v) for v in VALUES] for k in KEYS}}


if __name__ == "__main__":
    table = probe()
    if "--print" in sys.argv[1:]:
        json.dump(table, sys.stdout)
    else:
        compact = {"separators": (",", ":")}
        rows = ",\n".join(f'"{k}":{json.dumps(r, **compact)}' for k, r in table["returns"].items())   # one key per line
        with open(PATH, "w") as f:
            f.write(f'{{"values":{json.dumps(VALUES, **compact)},\n"returns":{{\n{rows}\n}}}}\n')
        print(f"wrote {PATH}: {len(table['returns'])} keys x {len(VALUES)} values")
