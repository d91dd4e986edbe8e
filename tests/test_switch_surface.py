"""The library's run-time switch surface, in source: every environment variable the library or the package reads
is a second product path, exercised only where something flips it.  So each one is in the table below with the reason it may stay -
a test that sets it, INTEGRATION.md documenting it as a setting, or a committed script that still sets a plain number - and the
table is checked against what the sources actually read.  A new switch fails this test until a test flips it; a retired one fails it
if it comes back (host only, no GPU)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dual-space-nerf_amd")
READS = re.compile(r'getenv\(\s*"(DSN\w*)"\s*\)|os\.environ\.get\(\s*"(DSN\w*)"|os\.environ\[\s*"(DSN\w*)"\s*\]')

# name -> (kind, where).  cross-check / capacity: `where` is a file of tests/ that sets the switch (a cross-check selects another kernel or
# branch whose result the test compares; a capacity makes a buffer or threshold small enough for a test-sized case to reach the other
# side); setting: user-facing, documented in INTEGRATION.md; tuning: a plain number that the committed script `where` still sets.
SWITCHES = {
    "DSN_WGRAD_PAIRS": ("cross-check", "tests/test_gpu_round5.py"),
    "DSN_TRAIN_LIN": ("cross-check", "tests/test_gpu_round5.py"),
    "DSN_TRAIN_UNFUSED_HEADS": ("cross-check", "tests/test_gpu_round5.py"),
    "DSN_TRAIN_ALL_ROWS": ("cross-check", "tests/test_gpu_round3.py"),
    "DSN_TRAIN_AUX": ("cross-check", "tests/test_gpu_round6.py"),
    "DSN_NN_UNFUSED": ("cross-check", "tests/test_gpu_round3.py"),
    "DSN_NN_NO_MEMBER": ("cross-check", "tests/test_gpu_round6.py"),
    "DSN_NN_NO_SUPER": ("cross-check", "tests/test_gpu_stages.py"),
    "DSN_NN_NO_CLEAR_CELLS": ("cross-check", "tests/test_gpu_clear_cells.py"),
    "DSN_FAR_SEGMENTS": ("cross-check", "tests/test_gpu_nns_block.py"),
    "DSN_SCREEN_WAVES": ("cross-check", "tests/test_gpu_field_bits.py"),
    "DSN_STOP_SLICE": ("cross-check", "tests/test_gpu_stop_slices.py"),
    "DSN_STOP_ADVANCE": ("cross-check", "tests/test_gpu_stop_slices.py"),
    "DSN_PERSISTENT_GROUPS": ("cross-check", "tests/test_gpu_tiles.py"),
    "DSN_NN_FINE_CAP": ("capacity", "tests/test_gpu_round4.py"),
    "DSN_RECORD_CAP": ("capacity", "tests/test_gpu_round2.py"),
    "DSN_CELLMAJOR_MIN": ("capacity", "tests/test_gpu_render.py"),
    "DSN_TRAIN_CELLMAJOR_MIN": ("capacity", "tests/test_gpu_round5.py"),
    "DSN_TRAIN_FAR_SEARCH_MIN": ("capacity", "tests/test_gpu_round3.py"),
    "DSN_POISON_SCRATCH": ("setting", "INTEGRATION.md"),
    "DSN_HOST_POOL": ("setting", "INTEGRATION.md"),
    "DSNERF_LIB": ("setting", "INTEGRATION.md"),
    "DSN_CALIB_BOX": ("tuning", "scripts/calib_probe.py"),
}

# switches that were measured once, kept their default and were flipped by no test: retired with the code only they reached
RETIRED = ["DSN_WGRAD16", "DSN_WGRAD_REDUCE", "DSN_WCOLSUM_ROWS", "DSN_TRAIN_COMPOSITE_ADJOINT", "DSN_TRAIN_HEADS", "DSN_TRAIN_COLSUM6",
           "DSN_TRAIN_SEED_MASK", "DSN_NN_ATOMIC_SCATTER", "DSN_LAZY_ALL_CELLS", "DSN_NN_FINE_TARGET", "DSN_FAR_SEG", "DSN_SHARE_EIGHTHS",
           "DSN_SCREEN_MARGIN", "DSN_TRAIN_FWD_AUX", "DSN_STOP_ROUND_ALPHA", "DSN_STOP_LAUNCH_ROUNDS"]


def _read(path):
    with open(path, errors="replace") as f:
        return f.read()


def _package_sources():
    files = glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.h"))
    files += glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True) + [os.path.join(ROOT, "dsnerf_amd.py")]
    return sorted(files)


def switches_read():
    """{name: [files that read it]} over the library's and the package's sources"""
    found = {}
    for path in _package_sources():
        for m in READS.finditer(_read(path)):
            found.setdefault(next(g for g in m.groups() if g), []).append(os.path.relpath(path, ROOT))
    return found


def test_every_switch_read_is_listed_with_what_keeps_it():
    found = switches_read()
    # the scan found the family it is about (a broken pattern cannot pass by matching nothing)
    assert set(found) >= {"DSN_WGRAD_PAIRS", "DSN_TRAIN_LIN", "DSN_TRAIN_UNFUSED_HEADS", "DSN_TRAIN_ALL_ROWS", "DSN_TRAIN_AUX", "DSN_NN_UNFUSED",
                          "DSN_NN_NO_MEMBER", "DSN_NN_NO_SUPER", "DSN_NN_NO_CLEAR_CELLS", "DSN_NN_FINE_CAP", "DSN_FAR_SEGMENTS",
                          "DSN_CELLMAJOR_MIN", "DSN_TRAIN_CELLMAJOR_MIN", "DSN_TRAIN_FAR_SEARCH_MIN", "DSN_RECORD_CAP", "DSN_STOP_SLICE",
                          "DSN_STOP_ADVANCE", "DSN_SCREEN_WAVES", "DSN_PERSISTENT_GROUPS", "DSN_CALIB_BOX", "DSN_POISON_SCRATCH",
                          "DSN_HOST_POOL", "DSNERF_LIB"}, sorted(found)
    unlisted = {k: v for k, v in found.items() if k not in SWITCHES}
    assert not unlisted, f"switches read by the sources and not listed here (a test has to flip a new switch): {unlisted}"
    gone = sorted(set(SWITCHES) - set(found))
    assert not gone, f"listed here and read nowhere any more: {gone}"
    for name, (kind, where) in SWITCHES.items():
        assert kind in ("cross-check", "capacity", "setting", "tuning"), (name, kind)
        if kind in ("cross-check", "capacity"):
            assert where.startswith("tests/") and where.endswith(".py"), (name, where)
        elif kind == "setting":
            assert where == "INTEGRATION.md", (name, where)
        else:
            assert where.startswith("scripts/"), (name, where)
        assert re.search(r"\b%s\b" % name, _read(os.path.join(ROOT, where))), f"{name}: {kind}, but {where} does not mention it"


def test_no_retired_switch_comes_back():
    assert not set(RETIRED) & set(SWITCHES)
    me = os.path.abspath(__file__)
    files = []
    for top in (PKG, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")):
        for ext in ("hip", "h", "py", "sh"):
            files += glob.glob(os.path.join(top, "**", "*." + ext), recursive=True)
    assert len(files) > 100
    hits = []
    for path in sorted(set(files)):
        if os.path.abspath(path) == me:
            continue
        text = _read(path)
        hits += [(os.path.relpath(path, ROOT), name) for name in RETIRED if re.search(r"\b%s\b" % name, text)]
    assert not hits, hits
