"""Every switch of the library has one row (kvcached_amd/csrc/options.cpp): option number, KVCACHED_* variable, default and
bounds. Here: what each numbered row loads from the environment at init and answers to set_option / get_option (on the "cpu"
device: the options are host state); the rows without a number in a native program under ASan + UBSan
(tests/native/options_check.cpp); and that the names of the numbers, the variables and their defaults are written once -
header = capi.py, library = INTEGRATION.md §5 = the table."""
import os
import re
import subprocess
from collections import namedtuple

import pytest

import kvc_testlib as T
from kvcached_amd import capi

# (option, variable, kind, default, min, max, shift, read-write) as the library has always behaved; min / max in the variable's units
Row = namedtuple("Row", "opt env kind default min max shift rw")
ROWS = [
    Row(capi.OPT_ZERO_BACKFILL, "KVCACHED_ZERO_BACKFILL", "bool", 1, None, None, 0, True),
    Row(capi.OPT_ZERO_FILL, "KVCACHED_ZERO_FILL", "bool", 1, None, None, 0, True),
    Row(capi.OPT_POOL_BYTES, "KVCACHED_PHYS_POOL_MB", "int", 16384, None, None, 20, True),
    Row(capi.OPT_PROFILE, None, "int", 0, None, None, 0, True),
    Row(capi.OPT_TLB_SHOOTDOWN, "KVCACHED_TLB_SHOOTDOWN", "bool", 1, None, None, 0, True),
    Row(capi.OPT_DEFER_UNMAP_SHOOTDOWN, "KVCACHED_DEFER_UNMAP_SHOOTDOWN", "bool", 0, None, None, 0, True),
    Row(capi.OPT_ASYNC_UNMAP, "KVCACHED_ASYNC_UNMAP", "bool", 0, None, None, 0, True),
    Row(capi.OPT_UNMAP_INVALIDATION_US, "KVCACHED_UNMAP_INVALIDATION_US", "int", 0, 0, None, 0, True),
    Row(capi.OPT_FILL_VARIANT, None, "int", 0, None, None, 0, True),
    Row(capi.OPT_COMPACT_VARIANT, None, "int", 0, None, None, 0, True),
    Row(capi.OPT_ACCESS_RUN_SLOTS, "KVCACHED_ACCESS_RUN_SLOTS", "int", 1, 1, None, 0, True),
    Row(capi.OPT_ZERO_ALIAS_FANOUT, "KVCACHED_ZERO_ALIAS_FANOUT", "int", 256, 1, None, 0, True),
    Row(capi.OPT_FILL_CHUNK_SLOTS, "KVCACHED_FILL_CHUNK_SLOTS", "int", 1024, 1, None, 0, True),
    Row(capi.OPT_POOL_IDLE_MS, "KVCACHED_POOL_IDLE_MS", "int", 1000, 0, None, 0, True),
    Row(capi.OPT_ASYNC_SHOOTDOWN, "KVCACHED_ASYNC_SHOOTDOWN", "bool", 1, None, None, 0, True),
    Row(capi.OPT_MAX_EXTENT_PAGES, "KVCACHED_PHYS_CHUNK_PAGES", "int", 1024, 1, 1024, 0, False),
]
ENV_ROWS = [r for r in ROWS if r.env]
RW_ROWS = [r for r in ROWS if r.rw]
# kvc_set_option stored whatever it was given for these two until they got their row: the lower bound the environment always
# had now holds through the C ABI as well (the one deliberate change of the table)
BOUND_NEW_ON_SET = (capi.OPT_ACCESS_RUN_SLOTS, capi.OPT_ZERO_ALIAS_FANOUT)
UNKNOWN_OPTION = 999


def _loaded(monkeypatch, row, text):
    """What get_option(row.opt) answers after an init with the row's variable set to `text` (None: unset)."""
    if text is None:
        monkeypatch.delenv(row.env, raising=False)
    else:
        monkeypatch.setenv(row.env, text)
    capi.init("cpu", 2 << 20, False)
    try:
        return capi.get_option(row.opt)
    finally:
        capi.shutdown()


@pytest.fixture
def clean_env(monkeypatch):
    for r in ENV_ROWS:
        monkeypatch.delenv(r.env, raising=False)
    yield monkeypatch
    for r in ENV_ROWS:
        monkeypatch.delenv(r.env, raising=False)
    capi.init("cpu", 2 << 20, False)   # the next test finds the defaults
    capi.shutdown()


@pytest.mark.parametrize("row", ENV_ROWS, ids=lambda r: r.env)
def test_init_loads_the_row_from_the_environment(clean_env, row):
    unit = 1 << row.shift
    assert _loaded(clean_env, row, None) == row.default * unit
    assert _loaded(clean_env, row, "") == row.default * unit
    if row.kind == "bool":
        for text in ("1", "true", "yes", "on", "TRUE"):
            assert _loaded(clean_env, row, text) == 1, text
        for text in ("0", "false", "off", "banana"):
            assert _loaded(clean_env, row, text) == 0, text
        return
    lo = 1 if row.min is None else row.min
    assert _loaded(clean_env, row, str(lo + 4)) == (lo + 4) * unit
    if row.min is not None:
        assert _loaded(clean_env, row, str(row.min - 1)) == row.min * unit
    else:
        assert _loaded(clean_env, row, "-3") == -3 * unit            # (no bounds today)
    if row.max is not None:
        assert _loaded(clean_env, row, str(row.max + 1)) == row.max * unit
    else:
        assert _loaded(clean_env, row, str(1 << 40)) == (1 << 40) * unit


def _round_trip(row, value):
    capi.set_option(row.opt, value)
    return capi.get_option(row.opt)


@pytest.mark.parametrize("row", RW_ROWS, ids=lambda r: str(r.env or r.opt))
def test_set_option_round_trips_and_clamps_by_the_row(clean_env, row):
    capi.init("cpu", 2 << 20, False)
    before = capi.get_option(row.opt)
    try:
        if row.kind == "bool":
            assert [_round_trip(row, v) for v in (0, 1, 0)] == [0, 1, 0]
            return
        lo = 1 if row.min is None else row.min
        for v in (lo, lo + 4, 1 << 40):                                # (set / get are in stored units: bytes for the pool)
            assert _round_trip(row, v) == v
        if row.min is None:
            assert _round_trip(row, -3) == -3
        elif row.opt not in BOUND_NEW_ON_SET:
            assert _round_trip(row, row.min - 1) == row.min and _round_trip(row, -(1 << 40)) == row.min
    finally:
        capi.set_option(row.opt, before)
        capi.shutdown()


@pytest.mark.parametrize("opt", BOUND_NEW_ON_SET)
def test_set_option_applies_the_lower_bound_the_environment_always_had(clean_env, opt):
    capi.init("cpu", 2 << 20, False)
    try:
        for v in (0, -7):
            capi.set_option(opt, v)
            assert capi.get_option(opt) == 1
    finally:
        capi.shutdown()


def test_read_only_and_unknown_numbers_are_refused(clean_env):
    capi.init("cpu", 2 << 20, False)
    try:
        for opt in (capi.OPT_MAX_EXTENT_PAGES, capi.OPT_EFFECTIVE_BACKEND, capi.OPT_SEG_MAP_IOCTLS, UNKNOWN_OPTION):
            assert capi.lib.kvc_set_option(opt, 1) == capi.KVC_E_INVALID
            assert capi.last_error() == "unknown option"
        assert capi.get_option(capi.OPT_MAX_EXTENT_PAGES) == 1024
        assert capi.lib.kvc_get_option(UNKNOWN_OPTION) == capi.KVC_E_INVALID and capi.last_error() == "unknown option"
        # every segment number answers (0 on the cpu device after a reset), the reserved ones included
        capi.reset_stats()
        assert [capi.get_option(o) for o in range(capi.OPT_HOST_SEGMENT_0, capi.OPT_SEG_END)] == [0] * 32
        assert capi.lib.kvc_get_option(capi.OPT_SEG_END) == capi.KVC_E_INVALID
    finally:
        capi.shutdown()


# ------------------------------------------------------------------ the rows without a number: native, under the sanitizers
@pytest.fixture(scope="module")
def options_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("native") / "options_check")
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-o", exe,
                           os.path.join(T.REPO, "tests", "native", "options_check.cpp"),
                           os.path.join(T.REPO, "kvcached_amd", "csrc", "options.cpp")], env=env)
    return lambda *args: subprocess.run([exe, *args], capture_output=True, text=True, timeout=120, env=env)


def test_rows_without_a_number_load_their_defaults_and_bounds(options_check):
    out = options_check()
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr[-3000:]


@pytest.fixture(scope="module")
def dumped(options_check):
    out = options_check("--dump")
    assert out.returncode == 0, out.stderr[-3000:]
    rows = {}
    for line in out.stdout.splitlines():
        name, default, lo, hi = line.split()
        rows[name] = (default, lo, hi)
    return rows


def test_the_dump_agrees_with_the_numbered_rows(dumped):
    for r in ENV_ROWS:
        default = {"bool": "true" if r.default else "false", "int": str(r.default)}[r.kind]
        bounds = ("-", "-") if r.kind == "bool" else tuple("-" if b is None else str(b) for b in (r.min, r.max))
        assert dumped[r.env] == (default,) + bounds, r.env


# ------------------------------------------------------------------ one source of truth
def _header_options():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(T.REPO, "include", "kvcached_amd.h")).read(), flags=re.S)
    return {name: int(n) for name, n in re.findall(r"\bKVC_OPT_([A-Z0-9_]+)\s*=\s*(\d+)", src)}


def test_capi_names_every_option_as_the_header_does():
    header = _header_options()
    mine = {k[4:]: v for k, v in vars(capi).items() if k.startswith("OPT_")}
    assert len(header) >= 60 and header == mine, sorted(set(header.items()) ^ set(mine.items()))


def _documented():
    """INTEGRATION.md §5's table: {variable: (default, 'C++' | 'Python')}."""
    text = open(os.path.join(T.REPO, "INTEGRATION.md")).read()
    rows = re.findall(r"^\s*\| `(KVCACHED_[A-Z0-9_]+)` \| `([^`]*)` \| (C\+\+|Python) \|", text, flags=re.M)
    assert len(rows) == len({r[0] for r in rows})
    return {name: (default, where) for name, default, where in rows}


def test_the_documented_switches_are_the_ones_in_the_shipped_library(dumped):
    with open(os.path.join(T.REPO, "kvcached_amd", "libkvcached_amd.so"), "rb") as f:
        shipped = {m.decode() for m in re.findall(rb"KVCACHED_[A-Z0-9_]+", f.read())}
    shipped = {n for n in shipped if not n.startswith("KVCACHED_AMD_")}
    doc = _documented()
    cxx = {n for n, (_, where) in doc.items() if where == "C++"}
    assert shipped == cxx, sorted(shipped ^ cxx)
    assert cxx == set(dumped), sorted(cxx ^ set(dumped))
    for name in sorted(cxx):
        assert doc[name][0] == dumped[name][0], name
    python_only = {n for n, (_, where) in doc.items() if where == "Python"}
    assert {"KVCACHED_TP_TRANSPORT", "KVCACHED_SHARED_POOL", "KVCACHED_BATCH_PAGE_ALLOC", "KVCACHED_HOST_CACHE_BLOCKS",
            "KVCACHED_HOST_CACHE_CODEC"} <= python_only


def _sources(*roots, suffixes):
    for root in roots:
        path = os.path.join(T.REPO, root)
        if os.path.isfile(path):
            yield path
        for d, _, files in os.walk(path):
            yield from (os.path.join(d, f) for f in files if f.endswith(suffixes))


def test_no_option_is_addressed_by_a_bare_number():
    call = re.compile(r"(?:get|set)_option\(\s*\d+")
    hits = []
    for path in _sources("tests", "benchmarks", "kvcached_amd", "tools_refresh_design_table.py", suffixes=(".py",)):
        for i, line in enumerate(open(path), 1):
            if call.search(line):
                hits.append(f"{os.path.relpath(path, T.REPO)}:{i}: {line.strip()}")
    unknown = [h for h in hits if h.startswith("tests/test_c_abi.py") and f"kvc_set_option({UNKNOWN_OPTION}, 1)" in h]
    assert len(unknown) == 1 and hits == unknown, hits


def test_no_option_or_segment_is_a_bare_number_in_the_library():
    bare = re.compile(r"case 1[0-9][0-9]\b|seg\[\d|\.mark\(\d")
    hits = [f"{os.path.relpath(p, T.REPO)}:{i}" for p in _sources("kvcached_amd/csrc", suffixes=(".cpp", ".hpp", ".hip", ".h"))
            for i, line in enumerate(open(p), 1) if bare.search(line)]
    assert not hits, hits
