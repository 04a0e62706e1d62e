"""The gemm tenant (operands global memory -> LDS -> MFMA) on a real MI355X:
the launch's checksum equals the closed form at one tile and one step, with
both LDS buffers, with an odd step count, at a tile count the XCDs do not
divide, over several passes, at the longest K and with whole groups of
tiles, unmasked and under the smallest mask; the default window measures
bf16 MFMAs; and two such tenants run as two processes.

Masks, children and their timeouts are handled as in test_gpu_mfma_lds.py.

The oracle is agent/cotenancy.py's gemm_checksum, closed form, itself checked
against a brute-force product in test_gemm_cotenancy_cpu.py. How large rate,
ratio, clock_ratio and cycle_ratio are is the result
(profiles/gemm_cotenancy_results.md), not a bound; the peak rate, the 2.4
GHz ceiling and the 32 cycles of a bf16 MFMA are derived."""
from __future__ import annotations

import pytest

from elastic_gpu_scheduler_amd.agent.cotenancy import gemm_checksum, isolation_report
from elastic_gpu_scheduler_amd.agent.cumask import CardMaskPlan, popcount

pytestmark = pytest.mark.gpu

SEED = 0x5EED
MAX_CLOCK_HZ = 2.4e9  # the shader clock's ceiling
MFMA_FLOP, MFMA_CYCLES = 32768, 32  # v_mfma_f32_32x32x16_bf16
# spread (max - min over five reports, 50 + 50 shares, default windows) of a
# gemm tenant's contended / solo ratio beside another gemm tenant: the margin
# by which a contended tenant may appear faster than alone
# (profiles/gemm_cotenancy_results.md).
GEMM_PAIR_SPREAD = 0.0104  # (0.0104, 0.0072)
DEFAULT_PASSES = 16
KEYS = ["kind", "applied_mask", "tick_hz", "workgroups", "m", "n", "k", "bytes", "passes",
        "checksum", "load_bytes_per_launch", "work_per_launch", "launches", "rate",
        "clock_ghz"]
LAUNCH_KEYS = ["t0", "t1", "seconds", "event_seconds", "rate", "cycles", "ticks",
               "clock_ghz"]
SHAPES = ((128, 64, 1), (128, 128, 1), (128, 192, 1), (384, 192, 1), (384, 320, 3),
          (128, 32768, 1), (1024, 256, 1))


@pytest.fixture(scope="module")
def probe():
    from elastic_gpu_scheduler_amd._native import gpuprobe

    p = gpuprobe()
    if p.device_count() == 0:
        pytest.fail("gpu-marked test ran but no HIP device is visible")
    return p


@pytest.fixture(scope="module")
def layout(probe):
    return probe.cu_mask_layout(0)


@pytest.fixture(scope="module")
def masks(layout):
    """The planner's masks; nothing masked is launched on another layout."""
    if not layout["interleaved"]:
        pytest.skip(f"CU-mask layout is not interleaved: {layout}")
    plan = CardMaskPlan(layout["cus"], layout["granule"])
    out = {"a50": plan.allocate("a", 50).mask, "b50": plan.allocate("b", 50).mask}
    out["tiny"] = CardMaskPlan(layout["cus"], layout["granule"]).allocate("t", 3).mask
    assert out["a50"] & out["b50"] == 0
    assert popcount(out["tiny"]) == layout["granule"]
    return out


def check(r, s, k, passes, mask, seed=SEED, launches=2):
    tiles = (s // 128) ** 2
    assert list(r) == KEYS
    assert len(r["launches"]) == launches
    assert all(list(l) == LAUNCH_KEYS for l in r["launches"])
    assert (r["kind"], r["m"], r["n"], r["k"], r["passes"]) == ("gemm", s, s, k, passes)
    assert r["bytes"] == 4 * s * k
    assert r["workgroups"] == tiles * passes
    assert r["work_per_launch"] == 2 * s * s * k * passes
    assert r["load_bytes_per_launch"] == tiles * passes * 2 * 128 * k * 2
    assert r["applied_mask"] == mask
    assert r["checksum"] == gemm_checksum(s, s, k, passes, seed), (s, k, passes, mask)


def run(probe, s, k, passes, **more):
    return probe.cu_tenant_run(0, kind="gemm", launches=2, bytes=4 * s * k, iters=k // 64,
                               passes=passes, **more)


@pytest.mark.parametrize("s,k,passes", SHAPES)
def test_checksum_equals_the_closed_form_unmasked(probe, s, k, passes):
    check(run(probe, s, k, passes, seed=SEED), s, k, passes, None)


@pytest.mark.parametrize("s,k,passes", ((384, 192, 1), (128, 192, 1)))
def test_checksum_equals_the_closed_form_one_granule(probe, masks, s, k, passes):
    """Under the smallest mask the workgroups queue for the CUs and their LDS."""
    r = run(probe, s, k, passes, seed=SEED, mask=masks["tiny"])
    check(r, s, k, passes, masks["tiny"])


def test_two_seeds_give_two_products(probe):
    a, b = (run(probe, 384, 192, 1, seed=seed) for seed in (SEED, SEED + 1))
    check(a, 384, 192, 1, None, seed=SEED)
    check(b, 384, 192, 1, None, seed=SEED + 1)
    assert a["checksum"] != b["checksum"]


def test_the_default_window_measures_bf16_mfmas(probe, layout):
    """Derived, none observed, as in test_gpu_mfma_lds.py: the rate stays
    below the bf16 peak at 2.4 GHz, and the cycles a SIMD spends per MFMA,
    from the clock the launch reports, cannot be fewer than 32. The 5 %
    below that is a condition, not a measurement; how far above a GEMM's
    loads and barriers put it is the result, and no upper bound is set."""
    r, cus = probe.cu_tenant_run(0, kind="gemm"), layout["cus"]
    check(r, 8192, 4096, DEFAULT_PASSES, None, seed=1, launches=8)
    peak_gflops = cus * 4 * (MFMA_FLOP / MFMA_CYCLES) * MAX_CLOCK_HZ / 1e9
    mfmas_per_simd = r["work_per_launch"] / MFMA_FLOP / (4 * cus)
    per_mfma = [l["clock_ghz"] * 1e9 * l["seconds"] / mfmas_per_simd for l in r["launches"]]
    print("gemm, rate:", r["rate"], "GFLOP/s of a peak of", peak_gflops, "clock_ghz:",
          r["clock_ghz"], "cycles per MFMA and SIMD:", [round(c, 3) for c in per_mfma])
    assert 0 < r["rate"] < peak_gflops
    assert all(0 < l["rate"] < peak_gflops for l in r["launches"])
    assert min(per_mfma) >= MFMA_CYCLES * 0.95, per_mfma


def test_two_processes_each_running_a_gemm(masks):
    """One report for two 50-share gemm tenants: alone (two children) and
    together (two more). The ratio and its split are the result, not a
    bound; asserted are their sanity and that both provably overlapped."""
    report = isolation_report(0, [{"mask": masks["a50"]}, {"mask": masks["b50"]}],
                              pairs=[("gemm", "gemm")], launches=8, timeout=120.0)
    print("50 + 50, gemm/gemm:", report)
    assert report["ok"], report  # children exited 0, checksums right, overlap
    for i, t in enumerate(report["pairs"]["gemm/gemm"]["tenants"]):
        solo = report["solo"][i]["gemm"]
        assert t["kind"] == "gemm" and t["contended_launches"] >= 3, t
        assert t["solo_rate"] == solo["rate"] and t["solo_clock_ghz"] == solo["clock_ghz"]
        assert t["clock_ratio"] > 0 and t["cycle_ratio"] > 0, t
        assert t["cycle_ratio"] * t["clock_ratio"] == pytest.approx(t["ratio"])
        assert 0 < t["ratio"] <= 1 + max(0.1, 2 * GEMM_PAIR_SPREAD), t
