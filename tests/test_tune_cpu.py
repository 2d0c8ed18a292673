"""CPU-only: the dgsct_test_tune switch table (csrc/tune.h), through the host emulation library, which links the same table
as libdgsct.so.  Defaults, set / restore, the clamp rules, the what-if gate -- and a source check that the C sources read no
environment variable but the documented eleven ("Switches")."""
import glob
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
from build_emu import build_emu  # noqa: E402

from dgsct_amd._lib import Lib  # noqa: E402

# key -> default.  gemmfx: 15 + 64 + 128 = 207 on the device, 31 + 64 + 128 = 223 in the emulation (bit 16, the prologues at every
# width: host loops have no tile economics)
DEFAULTS = {"gemm8": 1, "g8stag": 1, "gemmfx": 223, "wgbt": 1, "skinny": 1, "gemmtall": 1, "vq1fuse": 1, "gatefuse": 1, "rowfuse": 1,
            "bnfold": 1, "skfuse": 1, "callprof": 0, "skip": 0, "skipminc": 0, "skipmaxc": 1 << 30, "noatomic": 0}
WHATIF = ("skip", "skipminc", "skipmaxc", "noatomic")
ENV_KEPT = {"DGSCT_WIDE_ATTN", "DGSCT_GEMM_CFG", "DGSCT_GEMM_SPLITK", "DGSCT_PROF_DUMP", "DGSCT_CALL_PROF", "DGSCT_NO_GPROJ",
            "DGSCT_WHATIF", "DGSCT_GEMM8_GM", "DGSCT_GEMM8", "DGSCT_GEMM_SKINNY"}      # (DGSCT_NO_GPROJ: device and emulation)


@pytest.fixture(scope="module")
def emu():
    assert os.environ.get("DGSCT_WHATIF") != "1", "these tests need a process that has NOT opted in to the what-if switches"
    return Lib(build_emu())


@pytest.mark.parametrize("key", sorted(DEFAULTS))
def test_defaults(emu, key):
    assert emu.test_tune(key, -1) == DEFAULTS[key]


@pytest.mark.parametrize("key", [k for k in sorted(DEFAULTS) if k not in WHATIF])
def test_set_returns_old_value_and_restore(emu, key):
    old = emu.test_tune(key, 0)
    try:
        assert old == DEFAULTS[key]
        assert emu.test_tune(key, -1) == 0
        assert emu.test_tune(key, 1) == 0
        assert emu.test_tune(key, -1) == 1
    finally:
        assert emu.test_tune(key, old) in (0, 1)
    assert emu.test_tune(key, -1) == DEFAULTS[key]


@pytest.mark.parametrize("key,value,stored", [("gemmtall", 5, 1), ("gemmtall", 2, 2), ("vq1fuse", 3, 1), ("gatefuse", 2, 2),
                                              ("gemmfx", 0x1FF, 255), ("g8stag", 7, 1), ("wgbt", 2, 1), ("rowfuse", 2, 1),
                                              ("bnfold", 9, 1), ("skfuse", 2, 1), ("gemm8", 2, 2), ("skinny", 2, 2),
                                              ("callprof", 1, 1), ("callprof", 3, 0)])
def test_clamp_rules(emu, key, value, stored):
    old = emu.test_tune(key, value)
    try:
        assert emu.test_tune(key, -1) == stored
    finally:
        emu.test_tune(key, old)


def test_skipmaxc_zero_means_no_bound(emu):
    """(a what-if key: 0 may always be set)"""
    assert emu.test_tune("skipmaxc", 0) == 1 << 30
    assert emu.test_tune("skipmaxc", -1) == 1 << 30


@pytest.mark.parametrize("key", WHATIF)
def test_whatif_keys_need_the_opt_in(emu, key):
    assert emu.test_tune(key, 1) == -2
    assert "DGSCT_WHATIF" in emu.c.dgsct_last_error().decode()
    assert emu.test_tune(key, -1) == DEFAULTS[key]                  # nothing was stored; querying is always allowed
    assert emu.test_tune(key, 0) == DEFAULTS[key]                   # ... and so is switching it off


def test_unknown_key(emu):
    assert emu.test_tune("no-such-key", 1) == -1
    assert emu.test_tune("no-such-key", -1) == -1
    assert emu.test_tune("", -1) == -1


def test_whatif_opt_in_in_a_fresh_process(emu):
    code = ("import ctypes; c = ctypes.CDLL(%r); t = lambda k, v: c.dgsct_test_tune(k.encode(), v); "      # (plain ctypes: starts in milliseconds)
            "print(t('skip', 3), t('skip', -1), t('skipmaxc', 0), t('skipmaxc', 256), t('skipmaxc', -1), t('noatomic', 1), t('noatomic', 0))"
            % emu.path)
    env = dict(os.environ, DGSCT_WHATIF="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [0, 3, 1 << 30, 1 << 30, 256, 0, 1]


def _c_sources():
    return sorted([p for e in ("hip", "cpp", "h") for p in glob.glob(os.path.join(ROOT, "dg-sct_amd", "csrc", "*." + e))] + glob.glob(os.path.join(ROOT, "tests", "emu", "*.cpp")))


def test_only_the_documented_environment_variables_are_read():
    """every getenv in the C sources (a variable's name in the switch table of tune.h counts: it is what getenv gets there)"""
    names = set()
    for path in _c_sources():
        with open(path) as f:
            text = f.read()
        names.update(re.findall(r'getenv\(\s*"(DGSCT_\w+)"', text))
        if os.path.basename(path) == "tune.h":
            names.update(re.findall(r'"(DGSCT_\w+)"', text))
        assert "env_int" not in text, path
    assert names == ENV_KEPT


def test_no_mode_functions_left():
    for path in _c_sources():
        with open(path) as f:
            assert "_mode(int" not in f.read(), path
