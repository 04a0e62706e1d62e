"""The block-scaled gemm tenants (gemm-mxfp8, gemm-mxfp4: elements global
memory -> LDS -> MFMA, scales global memory -> registers, two slabs in
flight) on a real MI355X: the launch's checksum equals the closed form at
every prologue and epilogue of the distance-two pipeline, at a tile count
the XCDs do not divide, over several passes, at the form's longest K and
with whole bands of tiles, unmasked and under the smallest mask; the default
window measures the form's MFMAs; and two mxfp4 tenants run as two processes.

Masks, children and their timeouts are handled as in test_gpu_gemm_cotenancy.py.

The oracle is agent/cotenancy.py's gemm_checksum(form=), closed form, itself
checked against a brute-force product in test_mxgemm_cotenancy_cpu.py. How
large rate, ratio, clock_ratio and cycle_ratio are is the result
(profiles/mxgemm_cotenancy_results.md), not a bound; the peak rates, the 2.4
GHz ceiling and the 64 and 32 cycles of the two MFMAs are derived."""
from __future__ import annotations

import pytest

from elastic_gpu_scheduler_amd.agent.cotenancy import gemm_checksum, isolation_report
from elastic_gpu_scheduler_amd.agent.cumask import CardMaskPlan, popcount

pytestmark = pytest.mark.gpu

SEED = 0x5EED
MAX_CLOCK_HZ = 2.4e9  # the shader clock's ceiling
MFMA_FLOP = 131072    # v_mfma_scale_f32_32x32x64_f8f6f4
# kind: (form, k per step, scale bytes per row and step, most steps, cycles
# of one MFMA: 2 x and 4 x the bf16 rate of 1024 flop per cycle and SIMD)
FORMS = {"gemm-mxfp8": ("mxfp8", 128, 4, 256, 64), "gemm-mxfp4": ("mxfp4", 256, 8, 64, 32)}
# spread (max - min over five reports, 50 + 50 shares, default windows) of a
# gemm-mxfp4 tenant's contended / solo ratio beside another one: the margin
# by which a contended tenant may appear faster than alone
# (profiles/mxgemm_cotenancy_results.md).
MXGEMM_PAIR_SPREAD = 0.0056  # (0.0056, 0.0021)
DEFAULT_PASSES = {"gemm-mxfp8": 32, "gemm-mxfp4": 64}
KEYS = ["kind", "applied_mask", "tick_hz", "workgroups", "form", "m", "n", "k", "bytes",
        "scale_bytes", "passes", "checksum", "load_bytes_per_launch", "work_per_launch",
        "launches", "rate", "clock_ghz"]
LAUNCH_KEYS = ["t0", "t1", "seconds", "event_seconds", "rate", "cycles", "ticks",
               "clock_ghz"]
# (S, steps, passes); steps None: the form's most
SHAPES = ((128, 1, 1), (128, 2, 1), (128, 3, 1), (128, 4, 1), (128, 5, 1), (384, 3, 1),
          (384, 5, 3), (128, None, 1), (1024, 2, 1))


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


def check(r, kind, s, steps, passes, mask, seed=SEED, launches=2):
    form, step_k, word, _, _ = FORMS[kind]
    tiles, k = (s // 128) ** 2, step_k * steps
    assert list(r) == KEYS
    assert len(r["launches"]) == launches
    assert all(list(l) == LAUNCH_KEYS for l in r["launches"])
    assert (r["kind"], r["form"], r["m"], r["n"], r["k"], r["passes"]) == (
        kind, form, s, s, k, passes)
    assert r["bytes"] == 256 * s * steps == 2 * s * k * (8 if form == "mxfp8" else 4) // 8
    assert r["scale_bytes"] == 2 * steps * s * word
    assert r["workgroups"] == tiles * passes
    assert r["work_per_launch"] == 2 * s * s * k * passes
    assert r["load_bytes_per_launch"] == tiles * passes * steps * (32768 + 4 * 128 * word)
    assert r["applied_mask"] == mask
    assert r["checksum"] == gemm_checksum(s, s, k, passes, seed, form=form), (
        kind, s, steps, passes, mask)


def run(probe, kind, s, steps, passes, **more):
    return probe.cu_tenant_run(0, kind=kind, launches=2, bytes=256 * s * steps, iters=steps,
                               passes=passes, **more)


@pytest.mark.parametrize("s,steps,passes", SHAPES)
@pytest.mark.parametrize("kind", FORMS)
def test_checksum_equals_the_closed_form_unmasked(probe, kind, s, steps, passes):
    steps = steps or FORMS[kind][3]
    check(run(probe, kind, s, steps, passes, seed=SEED), kind, s, steps, passes, None)


@pytest.mark.parametrize("s,steps,passes", ((384, 3, 1), (128, 3, 1)))
@pytest.mark.parametrize("kind", FORMS)
def test_checksum_equals_the_closed_form_one_granule(probe, masks, kind, s, steps, passes):
    """Under the smallest mask the workgroups queue for the CUs and their LDS."""
    r = run(probe, kind, s, steps, passes, seed=SEED, mask=masks["tiny"])
    check(r, kind, s, steps, passes, masks["tiny"])


@pytest.mark.parametrize("kind", FORMS)
def test_two_seeds_give_two_products(probe, kind):
    a, b = (run(probe, kind, 384, 3, 1, seed=seed) for seed in (SEED, SEED + 1))
    check(a, kind, 384, 3, 1, None, seed=SEED)
    check(b, kind, 384, 3, 1, None, seed=SEED + 1)
    assert a["checksum"] != b["checksum"]


@pytest.mark.parametrize("kind", FORMS)
def test_the_default_window_measures_the_form_s_mfmas(probe, layout, kind):
    """Derived, none observed, as in test_gpu_gemm_cotenancy.py: the rate
    stays below the form's peak at 2.4 GHz, 2 x (mxfp8) or 4 x (mxfp4) the
    bf16 one, and the cycles a SIMD spends per MFMA, from the clock the
    launch reports, cannot be fewer than the instruction's 64 or 32. The 5 %
    below that is a condition, not a measurement; no upper bound is set."""
    cycles = FORMS[kind][4]
    r, cus = probe.cu_tenant_run(0, kind=kind), layout["cus"]
    check(r, kind, 8192, 4096 // FORMS[kind][1], DEFAULT_PASSES[kind], None, seed=1,
          launches=8)
    peak_gflops = cus * 4 * (MFMA_FLOP / cycles) * MAX_CLOCK_HZ / 1e9
    mfmas_per_simd = r["work_per_launch"] / MFMA_FLOP / (4 * cus)
    per_mfma = [l["clock_ghz"] * 1e9 * l["seconds"] / mfmas_per_simd for l in r["launches"]]
    print(kind, "passes:", r["passes"], "rate:", r["rate"], "GFLOP/s of a peak of",
          peak_gflops, "clock_ghz:", r["clock_ghz"], "launch seconds:",
          [l["seconds"] for l in r["launches"]], "cycles per MFMA and SIMD:",
          [round(c, 3) for c in per_mfma])
    assert 0 < r["rate"] < peak_gflops
    assert all(0 < l["rate"] < peak_gflops for l in r["launches"])
    assert min(per_mfma) >= cycles * 0.95, per_mfma


def test_two_processes_each_running_an_mxfp4_gemm(masks):
    """One report for two 50-share gemm-mxfp4 tenants: alone (two children)
    and together (two more). The ratio and its split are the result, not a
    bound; asserted are their sanity and that both provably overlapped."""
    kind = "gemm-mxfp4"
    report = isolation_report(0, [{"mask": masks["a50"]}, {"mask": masks["b50"]}],
                              pairs=[(kind, kind)], launches=8, timeout=120.0)
    print("50 + 50, gemm-mxfp4/gemm-mxfp4:", report)
    assert report["ok"], report  # children exited 0, checksums right, overlap
    for i, t in enumerate(report["pairs"][kind + "/" + kind]["tenants"]):
        solo = report["solo"][i][kind]
        assert t["kind"] == kind and t["contended_launches"] >= 3, t
        assert t["solo_rate"] == solo["rate"] and t["solo_clock_ghz"] == solo["clock_ghz"]
        assert t["clock_ratio"] > 0 and t["cycle_ratio"] > 0, t
        assert t["cycle_ratio"] * t["clock_ratio"] == pytest.approx(t["ratio"])
        assert 0 < t["ratio"] <= 1 + max(0.1, 2 * MXGEMM_PAIR_SPREAD), t
