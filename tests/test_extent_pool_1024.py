"""The physical-extent pool at extents of up to one bench batch (kMaxExtentPages = 1024 pages, 2 GiB of 2 MiB pages), on
the CPU: tests/native/extent_pool_1024_check.cpp, compiled with g++ under ASan + UBSan like tests/test_extent_pool.py. It
covers the handle tag (size and piece index up to 1024 x 1024 round-trip, foreign handles pass through), one 1024-page
extent taken apart and put back, and the footprint of request-shaped churn and of its adversary at 1024 against 64."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sanitizer_env():
    """The environment as it is, with two adjustments for a gcc ASan binary: whatever else is preloaded stays preloaded (so
    gcc's runtime cannot come first, and its link-order check is switched off), and only a clang sanitizer runtime - which
    tools_sanitize_cpu.sh preloads for its own builds and which would clash with gcc's - is left out of LD_PRELOAD."""
    env = dict(os.environ)
    if env.get("LD_PRELOAD"):
        libs = env["LD_PRELOAD"].replace(":", " ").split()
        keep = [p for p in libs if not os.path.basename(p).startswith("libclang_rt.")]
        if len(keep) != len(libs):
            env["LD_PRELOAD"] = " ".join(keep)
    env["ASAN_OPTIONS"] = ":".join(o for o in (env.get("ASAN_OPTIONS", ""), "verify_asan_link_order=0") if o)
    return env


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("native") / "extent_pool_1024_check")
    env = _sanitizer_env()
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-o", exe,
                           os.path.join(REPO, "tests", "native", "extent_pool_1024_check.cpp")], env=env)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]   # every REQUIRE in the program is an invariant
    return json.loads(out.stdout)


def test_every_size_and_index_up_to_1024_round_trips_through_the_tag(report):
    assert report["tag_round_trips"] == 4 * sum(range(2, 1025))


def test_one_extent_and_one_ioctl_per_bench_batch(report):
    assert report["bench_shape"]["creates"] == 1
    assert report["bench_shape"]["map_ioctls_per_page"] == pytest.approx(1 / 1024, rel=1e-3)


def test_request_shaped_churn_is_no_worse_at_1024_than_at_64(report):
    """(Requests of at most 40 pages never make an extent above 64 pages: this pins that the larger limit costs them nothing.)"""
    for name in ("requests", "requests_sorted_free_list"):
        k64, k1k = report[name + "_k64"], report[name + "_k1024"]
        assert k1k["p90"] <= 1.10, k1k
        assert k1k["p90"] <= k64["p90"] + 0.005 and k1k["held_over_mapped_p50"] <= k64["held_over_mapped_p50"] + 0.005


def test_the_adversary_is_no_worse_at_1024_than_at_64(report):
    for run in (32, 256):
        k64, k1k = report[f"tides_run{run}_k64"], report[f"tides_run{run}_k1024"]
        assert k1k["p90"] <= k64["p90"] + 0.005, (k64, k1k)


def test_bench_shaped_batches_with_stragglers_stay_within_a_few_points_of_64(report):
    """Runs of 256-1024 slots (longer than a 64-page extent) with 0 / 1 / 5 % of their pages freed on their own: here one
    straggler can pin a 2 GiB extent. The governor keeps the p90 within 3 points of the 64-page pool and below 1.10."""
    for pct in (0, 1, 5):
        k64, k1k = report[f"batches_straggle{pct}pct_k64"], report[f"batches_straggle{pct}pct_k1024"]
        assert k1k["p90"] <= 1.10 and k1k["p90"] <= k64["p90"] + 0.03, (pct, k64, k1k)
    assert report["batches_straggle0pct_k1024"]["max"] == 1.0
