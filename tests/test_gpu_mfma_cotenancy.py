"""The mfma tenant on a real MI355X: every lane's fold equals the closed
form on both sides of the chunk boundary, its launches are stamped sanely,
its shader-cycle record is consistent with the wall clock, what it measures
is the matrix pipe, and it runs as one of two processes next to another
mfma tenant and next to a 1 GiB streamer.

Every mask launched here comes from CardMaskPlan over the measured layout,
so it is a union of whole granules. If the layout does not come back
interleaved nothing masked is launched. Every child process has its own
timeout, and the first one that fails or times out ends the report it
belongs to: nothing further is started (agent/cotenancy.py).

The oracle is agent/cotenancy.py's mfma_checksum, pure Python and closed
form, itself checked against a brute-force model of the kernel in
test_mfma_cotenancy_cpu.py. How large ratio, clock_ratio and cycle_ratio are
is the result (profiles/mfma_cotenancy_results.md), not a bound. The upper
bands follow test_gpu_cotenancy.py: 1 + max(0.1, 2 x observed spread). The
peak rate, the 2.4 GHz ceiling of the clock, the 32 cycles of an MFMA and
the 8000 GB/s line are not observed but derived."""
from __future__ import annotations

import statistics

import pytest

from elastic_gpu_scheduler_amd.agent.cotenancy import isolation_report, mfma_checksum
from elastic_gpu_scheduler_amd.agent.cumask import CardMaskPlan, popcount

pytestmark = pytest.mark.gpu

SEED = 0x5EED
HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E peak; nothing read from HBM goes faster
MAX_CLOCK_HZ = 2.4e9    # the shader clock's ceiling
MFMA_FLOPS = 2 * 32 * 32 * 16  # one v_mfma_f32_32x32x16_bf16
MFMA_CYCLES = 32        # back-to-back issue of that MFMA on one SIMD
DEFAULT_ITERS = 32768

# spread (max - min over five reports, 50 + 50 shares, default windows) of a
# tenant's contended / solo ratio: the margin by which a contended tenant may
# appear faster than alone (profiles/mfma_cotenancy_results.md).
MFMA_PAIR_SPREAD = 0.0034           # an mfma tenant beside another (0.0012, 0.0034)
MFMA_BESIDE_STREAM_SPREAD = 0.0040  # an mfma tenant beside the 1 GiB streamer
STREAM_BESIDE_MFMA_SPREAD = 0.0183  # the streamer beside an mfma tenant


def half_width(spread: float) -> float:
    return max(0.1, 2 * spread)


@pytest.fixture(scope="module")
def probe():
    from elastic_gpu_scheduler_amd._native import gpuprobe

    p = gpuprobe()  # raises loudly if the HIP extension is missing
    if p.device_count() == 0:
        pytest.fail("gpu-marked test ran but no HIP device is visible")
    return p


@pytest.fixture(scope="module")
def layout(probe):
    lay = probe.cu_mask_layout(0)
    print("layout:", lay)
    return lay


@pytest.fixture(scope="module")
def masks(layout):
    """The planner's masks used below; skipped (nothing masked is launched)
    unless the card's layout is the interleaved one."""
    if not layout["interleaved"]:
        pytest.skip(f"CU-mask layout is not interleaved: {layout}")
    plan = CardMaskPlan(layout["cus"], layout["granule"])
    out = {"a50": plan.allocate("a", 50).mask, "b50": plan.allocate("b", 50).mask}
    out["tiny"] = CardMaskPlan(layout["cus"], layout["granule"]).allocate("t", 3).mask
    assert out["a50"] & out["b50"] == 0
    assert popcount(out["tiny"]) == layout["granule"]
    return out


def check(r, layout, iters, mask, seed=SEED):
    assert r["kind"] == "mfma" and r["iters"] == iters
    assert "bytes" not in r and "passes" not in r
    assert r["workgroups"] == 8 * layout["cus"]  # whatever the mask
    assert r["work_per_launch"] == 4 * r["workgroups"] * iters * 4 * MFMA_FLOPS
    assert r["applied_mask"] == mask
    assert r["checksum"] == mfma_checksum(r["workgroups"], iters, seed), (iters, mask)


# Both sides of the chunk boundary of 2048 steps, a single step, and an odd
# count that spans three chunks.
@pytest.mark.parametrize("iters", (1, 2, 2047, 2048, 2049, 4099))
def test_mfma_folds_equal_the_closed_form_unmasked(probe, layout, iters):
    r = probe.cu_tenant_run(0, kind="mfma", launches=2, iters=iters, seed=SEED)
    print(iters, "steps:", [l["seconds"] for l in r["launches"]])
    assert len(r["launches"]) == 2
    check(r, layout, iters, None)


@pytest.mark.parametrize("iters", (1, 2049))
def test_mfma_folds_equal_the_closed_form_one_granule(probe, layout, masks, iters):
    """The same under the smallest mask, where the eight fills queue for the
    CUs and a launch is about 32 x longer."""
    r = probe.cu_tenant_run(0, mask=masks["tiny"], kind="mfma", launches=2,
                            iters=iters, seed=SEED)
    print(iters, "steps:", [l["seconds"] for l in r["launches"]])
    assert len(r["launches"]) == 2
    check(r, layout, iters, masks["tiny"])


def test_mfma_defaults_iters_and_ignores_bytes_and_passes(probe, layout):
    r = probe.cu_tenant_run(0, kind="mfma", launches=1, iters=0, seed=SEED)
    check(r, layout, DEFAULT_ITERS, None)
    r = probe.cu_tenant_run(0, kind="mfma", launches=1, iters=3, bytes=12345,
                            passes=7, seed=SEED)
    check(r, layout, 3, None)


@pytest.fixture(scope="module")
def default_run(probe):
    """The default window, unmasked: 32768 steps, 8 launches."""
    return probe.cu_tenant_run(0, kind="mfma")


def test_mfma_stamps_are_sane(default_run, layout):
    r = default_run
    runs = r["launches"]
    print("seconds:", [l["seconds"] for l in runs],
          "event_seconds:", [l["event_seconds"] for l in runs],
          "clock_ghz:", [round(l["clock_ghz"], 4) for l in runs],
          "rate:", r["rate"], "tick_hz:", r["tick_hz"], "workgroups:", r["workgroups"])
    check(r, layout, DEFAULT_ITERS, None, seed=1)
    assert len(runs) == 8 and r["tick_hz"] > 0
    for l in runs:
        assert l["t0"] < l["t1"]
        assert l["seconds"] == pytest.approx((l["t1"] - l["t0"]) / r["tick_hz"])
        assert l["seconds"] <= l["event_seconds"]
        assert l["rate"] == pytest.approx(r["work_per_launch"] / l["seconds"] / 1e9)
        assert l["cycles"] > 0 and l["ticks"] > 0
        assert l["clock_ghz"] == pytest.approx(
            l["cycles"] / l["ticks"] * r["tick_hz"] / 1e9)
    for a, b in zip(runs, runs[1:]):
        assert a["t1"] <= b["t0"]
    assert r["rate"] == pytest.approx(statistics.median(l["rate"] for l in runs))
    assert r["clock_ghz"] == pytest.approx(
        statistics.median(l["clock_ghz"] for l in runs))


def test_it_is_the_matrix_pipe_that_is_measured(probe, default_run, layout):
    """Derived, none observed. A CU's four SIMDs each finish one 32768-flop
    MFMA per 32 cycles, 1024 flop per cycle and SIMD, at no more than 2.4
    GHz: 2516.6 TFLOP/s for 256 CUs. The cycle counter never runs faster
    than 2.4 GHz. And the cycles a SIMD spends per MFMA, from the clock the
    launch reports, cannot be fewer than 32: the 5 % below that is a
    condition, not a measurement, and claims nothing about performance; a
    factor of two in the flop or wave accounting, or a cycle counter that
    does not follow the shader clock, lands far outside it. The vector ALU's
    FP32 FMA does 256 flop per cycle and CU, a sixteenth of the bf16 matrix
    rate, so the fma kind must be slower."""
    r, cus = default_run, layout["cus"]
    peak_gflops = cus * 4 * (MFMA_FLOPS / MFMA_CYCLES) * MAX_CLOCK_HZ / 1e9
    mfmas_per_simd = r["work_per_launch"] / MFMA_FLOPS / (4 * cus)
    per_mfma = [l["clock_ghz"] * 1e9 * l["seconds"] / mfmas_per_simd
                for l in r["launches"]]
    print("rate:", r["rate"], "GFLOP/s of a peak of", peak_gflops,
          "clock_ghz:", r["clock_ghz"],
          "cycles per MFMA and SIMD:", [round(c, 3) for c in per_mfma])
    assert 0 < r["rate"] < peak_gflops
    for l in r["launches"]:
        assert 0 < l["rate"] < peak_gflops
        assert l["cycles"] <= MAX_CLOCK_HZ * (l["ticks"] + r["workgroups"]) / r["tick_hz"]
    assert min(per_mfma) >= MFMA_CYCLES * 0.95, per_mfma
    fma = probe.cu_tenant_run(0, kind="fma", launches=4)
    print("fma rate:", fma["rate"], "GFLOP/s")
    assert r["rate"] > fma["rate"] > 0


def report_for(masks, pair):
    report = isolation_report(
        0, [{"mask": masks["a50"]}, {"mask": masks["b50"]}],
        pairs=[pair], launches=8, timeout=120.0)
    print("50 + 50,", "/".join(pair) + ":", report)
    assert report.get("reason") != "child-failed", report
    return report


@pytest.fixture(scope="module")
def beside_another(masks):
    """One report for two 50-share mfma tenants: alone (two children) and
    together (two more)."""
    return report_for(masks, ("mfma", "mfma"))


@pytest.fixture(scope="module")
def beside_a_streamer(masks):
    """Likewise for an mfma tenant and the default 1 GiB x 127 streamer."""
    return report_for(masks, ("mfma", "stream"))


def check_split(t, solo):
    assert t["contended_launches"] >= 3, t
    for field in ("solo_clock_ghz", "contended_clock_ghz", "clock_ratio", "cycle_ratio"):
        assert t[field] > 0, (field, t)
    assert t["cycle_ratio"] * t["clock_ratio"] == pytest.approx(t["ratio"])
    assert t["clock_ratio"] == pytest.approx(
        t["contended_clock_ghz"] / t["solo_clock_ghz"])
    assert t["solo_rate"] == solo["rate"] and t["solo_clock_ghz"] == solo["clock_ghz"]


def test_two_processes_mfma_beside_mfma(beside_another):
    """The ratio and its split are the result (profiles/
    mfma_cotenancy_results.md), not a bound; asserted are their sanity and
    that both tenants provably overlapped."""
    report = beside_another
    assert report["ok"], report  # children exited 0, checksums right, overlap
    pair = report["pairs"]["mfma/mfma"]
    assert pair["ok"], pair
    for i, t in enumerate(pair["tenants"]):
        assert t["kind"] == "mfma"
        check_split(t, report["solo"][i]["mfma"])
        assert 0 < t["ratio"] <= 1 + half_width(MFMA_PAIR_SPREAD), t


def test_two_processes_mfma_beside_stream(beside_a_streamer):
    report = beside_a_streamer
    assert report["ok"], report
    pair = report["pairs"]["mfma/stream"]
    assert pair["ok"], pair
    mfma, stream = pair["tenants"]
    assert (mfma["kind"], stream["kind"]) == ("mfma", "stream")
    check_split(mfma, report["solo"][0]["mfma"])
    assert 0 < mfma["ratio"] <= 1 + half_width(MFMA_BESIDE_STREAM_SPREAD), mfma
    assert stream["contended_launches"] >= 3, stream
    assert 0 < stream["ratio"] <= 1 + half_width(STREAM_BESIDE_MFMA_SPREAD), stream
    assert not any(f in stream for f in ("solo_clock_ghz", "contended_clock_ghz",
                                         "clock_ratio", "cycle_ratio"))
    assert 0 < stream["contended_rate"] < HBM_PEAK_GBPS, stream
    assert 0 < stream["solo_rate"] < HBM_PEAK_GBPS, stream
    assert stream["solo_rate"] == report["solo"][1]["stream"]["rate"]
