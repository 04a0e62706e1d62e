"""The gemm tenant with loads="direct" on a real MI355X: the closed form with
one to five steps (fewer than the ring is deep, its first wrap, one past it,
for a ring of two or three), 9 tiles, several passes, the longest K and whole
bands of tiles; the smallest mask; both load paths; the default window; two
processes. Masks, fixtures and derived bounds are test_gpu_gemm_cotenancy.py's;
the figures are the result (profiles/gemm_direct_cotenancy_results.md)."""
from __future__ import annotations

import pytest

from elastic_gpu_scheduler_amd.agent.cotenancy import gemm_checksum, isolation_report
from tests.test_gpu_gemm_cotenancy import (KEYS, LAUNCH_KEYS, MAX_CLOCK_HZ, MFMA_CYCLES,
                                           MFMA_FLOP, SEED, layout, masks, probe)  # noqa: F401

pytestmark = pytest.mark.gpu

STAGES = 2  # the build's kGemmDirectStages
# max - min of a tenant's ratio over five reports (the profile named above)
DIRECT_PAIR_SPREAD = 0.0609  # (0.0421, 0.0609)
DIRECT_KEYS = KEYS[:11] + ["loads", "stages", "lds_bytes"] + KEYS[11:]  # after load_bytes_...
SHAPES = ((128, 64, 1), (128, 128, 1), (128, 192, 1), (128, 256, 1), (128, 320, 1),
          (384, 192, 1), (384, 320, 3), (128, 32768, 1), (1024, 256, 1))


def run(probe, s, k, passes, loads="direct", **more):
    return probe.cu_tenant_run(0, kind="gemm", launches=2, bytes=4 * s * k, iters=k // 64,
                               passes=passes, loads=loads, **more)


def check(r, s, k, passes, mask, seed=SEED, launches=2):
    assert list(r) == DIRECT_KEYS
    assert all(list(l) == LAUNCH_KEYS for l in r["launches"]) and len(r["launches"]) == launches
    assert (r["kind"], r["m"], r["n"], r["k"], r["passes"]) == ("gemm", s, s, k, passes)
    assert (r["loads"], r["stages"], r["lds_bytes"]) == ("direct", STAGES, STAGES * 32768 + 2048)
    assert r["workgroups"] == (s // 128) ** 2 * passes and r["applied_mask"] == mask
    assert r["load_bytes_per_launch"] == r["workgroups"] * 2 * 128 * k * 2
    assert r["checksum"] == gemm_checksum(s, s, k, passes, seed), (s, k, passes, mask)


@pytest.mark.parametrize("s,k,passes", SHAPES)
def test_checksum_equals_the_closed_form_unmasked(probe, s, k, passes):
    check(run(probe, s, k, passes, seed=SEED), s, k, passes, None)


@pytest.mark.parametrize("s,k,passes", ((384, 192, 1), (128, 192, 1)))
def test_checksum_equals_the_closed_form_one_granule(probe, masks, s, k, passes):
    check(run(probe, s, k, passes, seed=SEED, mask=masks["tiny"]), s, k, passes, masks["tiny"])


def test_two_seeds_give_two_products_and_both_paths_the_same(probe):
    a, b = (run(probe, 384, 192, 1, seed=seed) for seed in (SEED, SEED + 1))
    check(a, 384, 192, 1, None, seed=SEED)
    check(b, 384, 192, 1, None, seed=SEED + 1)
    assert a["checksum"] != b["checksum"]
    staged = run(probe, 384, 192, 1, loads="registers", seed=SEED)
    assert list(staged) == KEYS and staged["checksum"] == a["checksum"]


def test_the_default_window_measures_bf16_mfmas(probe, layout):
    """Derived bounds, as in test_gpu_gemm_cotenancy.py; no upper bound."""
    r, cus = probe.cu_tenant_run(0, kind="gemm", loads="direct"), layout["cus"]
    check(r, 8192, 4096, 16, None, seed=1, launches=8)
    peak_gflops = cus * 4 * (MFMA_FLOP / MFMA_CYCLES) * MAX_CLOCK_HZ / 1e9
    mfmas_per_simd = r["work_per_launch"] / MFMA_FLOP / (4 * cus)
    per_mfma = [l["clock_ghz"] * 1e9 * l["seconds"] / mfmas_per_simd for l in r["launches"]]
    print("gemm direct, rate:", r["rate"], "GFLOP/s of a peak of", peak_gflops, "clock_ghz:",
          r["clock_ghz"], "cycles per MFMA and SIMD:", [round(c, 3) for c in per_mfma])
    assert 0 < r["rate"] < peak_gflops
    assert all(0 < l["rate"] < peak_gflops for l in r["launches"])
    assert min(per_mfma) >= MFMA_CYCLES * 0.95, per_mfma


def test_two_processes_each_running_a_direct_gemm(masks):
    report = isolation_report(0, [{"mask": masks["a50"]}, {"mask": masks["b50"]}],
                              pairs=[("gemm", "gemm")], launches=8, loads="direct")
    print("50 + 50, gemm/gemm, direct:", report)
    assert report["ok"], report  # children exited 0, checksums right, overlap
    for i, t in enumerate(report["pairs"]["gemm/gemm"]["tenants"]):
        assert t["loads"] == report["solo"][i]["gemm"]["loads"] == "direct"
        assert t["contended_launches"] >= 3 and t["clock_ratio"] > 0 and t["cycle_ratio"] > 0
        assert t["cycle_ratio"] * t["clock_ratio"] == pytest.approx(t["ratio"])
        assert 0 < t["ratio"] <= 1 + max(0.1, 2 * DIRECT_PAIR_SPREAD), t
