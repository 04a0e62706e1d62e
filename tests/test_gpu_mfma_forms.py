"""The forms of the mfma tenant (fp8, mxfp8, mxfp4 beside bf16) on a real
MI355X: every lane's fold equals the form's closed form on both sides of the
form's chunk boundary, the defaults are the form's, what each form measures
is its own matrix instruction, and the forms run as one of two processes:
mxfp4 beside mxfp4, and bf16 beside mxfp4.

Every mask launched here comes from CardMaskPlan over the measured layout,
so it is a union of whole granules. If the layout does not come back
interleaved nothing masked is launched. Every child process has its own
timeout, and the first one that fails or times out ends the report it
belongs to: nothing further is started (agent/cotenancy.py).

The oracle is agent/cotenancy.py's mfma_checksum(form=...), pure Python and
closed form, itself checked against a brute-force model of the kernel in
test_mfma_forms_cpu.py. How large ratio, clock_ratio and cycle_ratio are is
the result (profiles/mfma_forms_cotenancy_results.md), not a bound. The
upper bands follow test_gpu_mfma_cotenancy.py: 1 + max(0.1, 2 x observed
spread). The peak rates, the 2.4 GHz ceiling of the clock and the cycles of
an MFMA of each form are not observed but derived."""
from __future__ import annotations

import pytest

from elastic_gpu_scheduler_amd.agent.cotenancy import isolation_report, mfma_checksum
from elastic_gpu_scheduler_amd.agent.cumask import CardMaskPlan, popcount

pytestmark = pytest.mark.gpu

SEED = 0x5EED
MAX_CLOCK_HZ = 2.4e9  # the shader clock's ceiling
FORMS = ("bf16", "fp8", "mxfp8", "mxfp4")
NEW_FORMS = FORMS[1:]
# form: (K, flop per MFMA, chunk, default iters, cycles of one MFMA issued
# back to back on one SIMD). The cycles are the spec's dense 2.5 / 2.5 / 5 /
# 10 PFLOP/s at 2.4 GHz over 256 CUs x 4 SIMDs: fp8 the cycles of bf16 at
# the same K, mxfp8 twice them at 4 x the K, mxfp4 the same at 4 x the K.
RULES = {
    "bf16": (16, 32768, 2048, 32768, 32),
    "fp8": (16, 32768, 2048, 32768, 32),
    "mxfp8": (64, 131072, 512, 16384, 64),
    "mxfp4": (64, 131072, 256, 32768, 32),
}

# spread (max - min over five reports, 50 + 50 shares, default windows) of a
# tenant's contended / solo ratio: the margin by which a contended tenant may
# appear faster than alone (profiles/mfma_forms_cotenancy_results.md).
MXFP4_PAIR_SPREAD = 0.0027         # an mxfp4 tenant beside another (0.0027, 0.0022)
BF16_BESIDE_MXFP4_SPREAD = 0.0050  # a bf16 tenant beside an mxfp4 one (0.0030, 0.0050)
MXFP4_BESIDE_BF16_SPREAD = 0.0110  # an mxfp4 tenant beside a bf16 one (0.0037, 0.0110)


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


def check(r, layout, form, iters, mask, seed=SEED):
    assert r["kind"] == "mfma" and r["form"] == form and r["iters"] == iters
    assert "bytes" not in r and "passes" not in r
    assert r["workgroups"] == 8 * layout["cus"]  # whatever the mask
    assert r["work_per_launch"] == 4 * r["workgroups"] * iters * 4 * RULES[form][1]
    assert r["applied_mask"] == mask
    assert r["checksum"] == mfma_checksum(r["workgroups"], iters, seed, form), (
        form, iters, mask)


# A single step, two, both sides of the form's chunk boundary, and an odd
# count that spans three chunks: position 0..5 of that list.
@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("form", NEW_FORMS)
def test_form_folds_equal_the_closed_form_unmasked(probe, layout, form, which):
    chunk = RULES[form][2]
    iters = (1, 2, chunk - 1, chunk, chunk + 1, 2 * chunk + 3)[which]
    r = probe.cu_tenant_run(0, kind="mfma", launches=2, iters=iters, seed=SEED, form=form)
    print(form, iters, "steps:", [l["seconds"] for l in r["launches"]])
    assert len(r["launches"]) == 2
    check(r, layout, form, iters, None)


@pytest.mark.parametrize("past_a_chunk", (False, True))
@pytest.mark.parametrize("form", NEW_FORMS)
def test_form_folds_equal_the_closed_form_one_granule(probe, layout, masks, form,
                                                      past_a_chunk):
    """The same under the smallest mask, where the eight fills queue for the
    CUs: one step, and one step past the form's chunk."""
    iters = RULES[form][2] + 1 if past_a_chunk else 1
    r = probe.cu_tenant_run(0, mask=masks["tiny"], kind="mfma", launches=2,
                            iters=iters, seed=SEED, form=form)
    print(form, iters, "steps:", [l["seconds"] for l in r["launches"]])
    assert len(r["launches"]) == 2
    check(r, layout, form, iters, masks["tiny"])


@pytest.mark.parametrize("form", FORMS)
def test_form_defaults_its_iters(probe, layout, form):
    r = probe.cu_tenant_run(0, kind="mfma", launches=1, iters=0, seed=SEED, form=form)
    check(r, layout, form, RULES[form][3], None)


def test_bf16_is_what_no_form_runs(probe, layout):
    r = probe.cu_tenant_run(0, kind="mfma", launches=1, iters=3, seed=SEED)
    check(r, layout, "bf16", 3, None)
    assert r["checksum"] == mfma_checksum(r["workgroups"], 3, SEED)


@pytest.fixture(scope="module")
def default_runs(probe):
    """Per form the default window, unmasked: the form's default steps, 8
    launches, seed 1."""
    return {form: probe.cu_tenant_run(0, kind="mfma", form=form) for form in FORMS}


@pytest.mark.parametrize("form", FORMS)
def test_it_is_the_form_s_instruction_that_is_measured(default_runs, layout, form):
    """Derived, none observed. A CU's four SIMDs each finish one MFMA of the
    form's flop per the form's cycles, at no more than 2.4 GHz: 2.5, 2.5, 5
    and 10 PFLOP/s for 256 CUs. And the cycles a SIMD spends per MFMA, from
    the clock the launch reports, cannot be fewer than the form's: the 5 %
    below that is a condition, not a measurement, and claims nothing about
    performance; a form sent to another form's instruction, or a factor of
    two in the flop accounting, lands far outside it."""
    r, cus = default_runs[form], layout["cus"]
    _, flop, _, iters, cycles = RULES[form]
    check(r, layout, form, iters, None, seed=1)
    peak_gflops = cus * 4 * (flop / cycles) * MAX_CLOCK_HZ / 1e9
    mfmas_per_simd = r["work_per_launch"] / flop / (4 * cus)
    per_mfma = [l["clock_ghz"] * 1e9 * l["seconds"] / mfmas_per_simd
                for l in r["launches"]]
    print(form, "rate:", r["rate"], "GFLOP/s of a peak of", peak_gflops,
          "clock_ghz:", r["clock_ghz"],
          "cycles per MFMA and SIMD:", [round(c, 3) for c in per_mfma])
    assert len(r["launches"]) == 8
    assert 0 < r["rate"] < peak_gflops
    for l in r["launches"]:
        assert 0 < l["rate"] < peak_gflops
    assert min(per_mfma) >= cycles * 0.95, per_mfma


def test_flop_per_cycle_orders_the_forms(default_runs):
    """Flop per shader cycle: derived 4 x bf16 for mxfp4 and 2 x for mxfp8,
    so a form sent to the wrong instruction lands a factor of two away and
    no fold overhead can invert the order. fp8 is derived equal to bf16 and
    is not ordered against it."""
    per_cycle = {form: r["rate"] / r["clock_ghz"] for form, r in default_runs.items()}
    print("GFLOP/s per GHz:", per_cycle)
    assert per_cycle["mxfp4"] > per_cycle["mxfp8"] > per_cycle["bf16"] > 0
    assert per_cycle["fp8"] > 0


def report_for(masks, forms=(None, None), form=None):
    tenants = [{"mask": masks[m], **({"form": f} if f else {})}
               for m, f in zip(("a50", "b50"), forms)]
    report = isolation_report(0, tenants, pairs=[("mfma", "mfma")], launches=8,
                              timeout=120.0, form=form)
    print("50 + 50, mfma/mfma,", forms, form, ":", report)
    assert report.get("reason") != "child-failed", report
    return report


@pytest.fixture(scope="module")
def mxfp4_beside_mxfp4(masks):
    """One report for two 50-share mxfp4 tenants: alone (two children) and
    together (two more)."""
    return report_for(masks, form="mxfp4")


@pytest.fixture(scope="module")
def bf16_beside_mxfp4(masks):
    """Likewise for a bf16 tenant and an mxfp4 one, each tenant its own form."""
    return report_for(masks, forms=("bf16", "mxfp4"))


def check_split(t, solo):
    assert t["contended_launches"] >= 3, t
    for field in ("solo_clock_ghz", "contended_clock_ghz", "clock_ratio", "cycle_ratio"):
        assert t[field] > 0, (field, t)
    assert t["cycle_ratio"] * t["clock_ratio"] == pytest.approx(t["ratio"])
    assert t["clock_ratio"] == pytest.approx(
        t["contended_clock_ghz"] / t["solo_clock_ghz"])
    assert t["solo_rate"] == solo["rate"] and t["solo_clock_ghz"] == solo["clock_ghz"]


def test_two_processes_mxfp4_beside_mxfp4(mxfp4_beside_mxfp4):
    """The ratio and its split are the result (profiles/
    mfma_forms_cotenancy_results.md), not a bound; asserted are their sanity
    and that both tenants provably overlapped."""
    report = mxfp4_beside_mxfp4
    assert report["ok"], report  # children exited 0, checksums right, overlap
    pair = report["pairs"]["mfma/mfma"]
    assert pair["ok"], pair
    for i, t in enumerate(pair["tenants"]):
        assert t["kind"] == "mfma" and t["form"] == "mxfp4"
        assert report["solo"][i]["mfma"]["form"] == "mxfp4"
        check_split(t, report["solo"][i]["mfma"])
        assert 0 < t["ratio"] <= 1 + half_width(MXFP4_PAIR_SPREAD), t


def test_two_processes_bf16_beside_mxfp4(bf16_beside_mxfp4):
    report = bf16_beside_mxfp4
    assert report["ok"], report
    pair = report["pairs"]["mfma/mfma"]
    assert pair["ok"], pair
    spreads = (BF16_BESIDE_MXFP4_SPREAD, MXFP4_BESIDE_BF16_SPREAD)
    for i, form in enumerate(("bf16", "mxfp4")):
        t = pair["tenants"][i]
        assert t["kind"] == "mfma" and t["form"] == form
        assert report["solo"][i]["mfma"]["form"] == form
        check_split(t, report["solo"][i]["mfma"])
        assert 0 < t["ratio"] <= 1 + half_width(spreads[i]), t
