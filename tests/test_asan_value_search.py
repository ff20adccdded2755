"""Host AddressSanitizer + UBSan run of the native search's value mode
(AZG_MCTS_SEARCH_VALUE): mcts_engine.cpp compiled whole with -fsanitize and driven through
its C-ABI by the stand-alone csrc/asan/asan_mcts_value_main.cpp -- collisions, final
flushes, noise on an existing root, clear, bad arguments.  Any sanitizer report fails the
test.  CPU only; the binary runs on its own (nothing is preloaded, no Python inside)."""
import os
import subprocess

import pytest

from conftest import PKG

CSRC = os.path.join(PKG, "csrc")
DRIVER = "asan_mcts_value"


@pytest.fixture(scope="module")
def built():
    r = subprocess.run(["make", "-C", CSRC, f"build_asan/{DRIVER}"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return os.path.join(CSRC, "build_asan")


@pytest.mark.timeout(300)
def test_sanitized_value_search_driver(built):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(built, DRIVER)], capture_output=True, text=True, timeout=240, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-3000:]
    assert f"{DRIVER}: ok" in out
