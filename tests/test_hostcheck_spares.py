"""The cache policy of a decode context (draco-sharp_amd/csrc/dsa_spares.h: best fit, three blocks kept, the caches that give way
before an allocation is tried again, the arena's last resort) compiled for the host over malloc / free under AddressSanitizer +
UBSan with leak detection on (tests/hostcheck/spares_host.cpp): every row of the table of blocks a batch takes, with none, the
first, the first two and every allocation failing, and two threads on one cache.  A check of the product source on CPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "spares_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("spares") / "spares_host")      # always rebuilt: the source under test changes
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread", "-o", out, SRC], check=True)
    return out


def test_cache_policy(exe):
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "LSAN_OPTIONS")}      # leak detection stays on
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "spares: best fit, three kept, 6 rows x 4 failure counts, two threads" in r.stdout and "each released once" in r.stdout
