"""The mfma tenant with its operands re-read from LDS (operands="lds") on a
real MI355X: every lane's fold equals the closed form at every remainder of
the slot rotation and on both sides of the form's chunk boundary, unmasked
and under the smallest mask; one step equals the run from registers and two
do not; the default window of every form measures the form's instruction;
and two such tenants run as two processes, bf16 beside bf16 and mxfp4 beside
mxfp4.

Every mask launched here comes from CardMaskPlan over the measured layout,
so it is a union of whole granules. If the layout does not come back
interleaved nothing masked is launched. Every child process has its own
timeout, and the first one that fails or times out ends the report it
belongs to: nothing further is started (agent/cotenancy.py).

The oracle is agent/cotenancy.py's mfma_checksum(..., operands="lds"), pure
Python and closed form, itself checked against a brute-force model of the
kernel in test_mfma_lds_cpu.py. How large ratio, clock_ratio and cycle_ratio
are, and how many cycles an MFMA takes with its operands coming from LDS, is
the result (profiles/mfma_lds_cotenancy_results.md), not a bound. The upper
bands follow test_gpu_mfma_forms.py: 1 + max(0.1, 2 x observed spread). The
peak rates, the 2.4 GHz ceiling of the clock and the cycles of an MFMA of
each form are not observed but derived."""
from __future__ import annotations

import pytest

from elastic_gpu_scheduler_amd.agent.cotenancy import (MFMA_LDS_SLOTS,
                                                       MFMA_LDS_STEP_BYTES,
                                                       isolation_report, mfma_checksum)
from elastic_gpu_scheduler_amd.agent.cumask import CardMaskPlan, popcount

pytestmark = pytest.mark.gpu

SEED = 0x5EED
MAX_CLOCK_HZ = 2.4e9  # the shader clock's ceiling
FORMS = ("bf16", "fp8", "mxfp8", "mxfp4")
# form: (K, flop per MFMA, chunk, default iters, cycles of one MFMA issued
# back to back on one SIMD), as in test_gpu_mfma_forms.py.
RULES = {
    "bf16": (16, 32768, 2048, 32768, 32),
    "fp8": (16, 32768, 2048, 32768, 32),
    "mxfp8": (64, 131072, 512, 16384, 64),
    "mxfp4": (64, 131072, 256, 32768, 32),
}

# spread (max - min over five reports, 50 + 50 shares, default windows, both
# tenants with operands from LDS) of a tenant's contended / solo ratio: the
# margin by which a contended tenant may appear faster than alone
# (profiles/mfma_lds_cotenancy_results.md).
BF16_LDS_PAIR_SPREAD = 0.0013   # a bf16 tenant beside another (0.0013, 0.0010)
MXFP4_LDS_PAIR_SPREAD = 0.0023  # an mxfp4 tenant beside another (0.0015, 0.0023)


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
    assert r["operands"] == "lds"
    assert "bytes" not in r and "passes" not in r
    assert r["workgroups"] == 8 * layout["cus"]  # whatever the mask
    assert r["work_per_launch"] == 4 * r["workgroups"] * iters * 4 * RULES[form][1]
    assert r["lds_bytes"] == MFMA_LDS_SLOTS * MFMA_LDS_STEP_BYTES[form]
    assert r["lds_bytes_per_launch"] == (
        4 * r["workgroups"] * iters * MFMA_LDS_STEP_BYTES[form])
    assert r["applied_mask"] == mask
    assert r["checksum"] == mfma_checksum(r["workgroups"], iters, seed, form, "lds"), (
        form, iters, mask)


# Every remainder of the slot rotation twice over, both sides of the form's
# chunk boundary, and an odd count that spans three chunks: position 0..8.
@pytest.mark.parametrize("which", range(9))
@pytest.mark.parametrize("form", FORMS)
def test_lds_folds_equal_the_closed_form_unmasked(probe, layout, form, which):
    chunk = RULES[form][2]
    iters = (1, 2, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 3)[which]
    r = probe.cu_tenant_run(0, kind="mfma", launches=2, iters=iters, seed=SEED,
                            form=form, operands="lds")
    print(form, iters, "steps:", [l["seconds"] for l in r["launches"]])
    assert len(r["launches"]) == 2
    check(r, layout, form, iters, None)


@pytest.mark.parametrize("past_a_chunk", (False, True))
@pytest.mark.parametrize("form", FORMS)
def test_lds_folds_equal_the_closed_form_one_granule(probe, layout, masks, form,
                                                     past_a_chunk):
    """The same under the smallest mask, where the workgroups queue for the
    CUs and for their LDS: two steps, and one step past the form's chunk."""
    iters = RULES[form][2] + 1 if past_a_chunk else 2
    r = probe.cu_tenant_run(0, mask=masks["tiny"], kind="mfma", launches=2,
                            iters=iters, seed=SEED, form=form, operands="lds")
    print(form, iters, "steps:", [l["seconds"] for l in r["launches"]])
    assert len(r["launches"]) == 2
    check(r, layout, form, iters, masks["tiny"])


@pytest.mark.parametrize("form", FORMS)
def test_one_step_from_lds_equals_one_step_from_registers(probe, form):
    """With one step every wave multiplies its own variant, read back from
    the slot it wrote; with two it multiplies its neighbour's as well."""
    def run(iters, operands):
        return probe.cu_tenant_run(0, kind="mfma", launches=1, iters=iters, seed=SEED,
                                   form=form, operands=operands)

    lds, registers = run(1, "lds"), run(1, "registers")
    assert lds["checksum"] == registers["checksum"]
    assert lds["operands"] == "lds"
    for key in ("operands", "lds_bytes", "lds_bytes_per_launch"):
        assert key not in registers
    assert run(2, "lds")["checksum"] != run(2, "registers")["checksum"]


@pytest.fixture(scope="module")
def default_runs(probe):
    """Per form the default window, unmasked, operands from LDS: the form's
    default steps, 8 launches, seed 1."""
    return {form: probe.cu_tenant_run(0, kind="mfma", form=form, operands="lds")
            for form in FORMS}


@pytest.mark.parametrize("form", FORMS)
def test_it_is_the_form_s_instruction_that_is_measured_from_lds(default_runs, layout,
                                                                form):
    """Derived, none observed, as in test_gpu_mfma_forms.py: the rate stays
    below the form's peak at 2.4 GHz, and the cycles a SIMD spends per MFMA,
    from the clock the launch reports, cannot be fewer than the form's. The
    5 % below that is a condition, not a measurement, and claims nothing
    about performance: how many cycles the LDS reads add is the result
    (profiles/mfma_lds_cotenancy_results.md), and no upper bound is set."""
    r, cus = default_runs[form], layout["cus"]
    _, flop, _, iters, cycles = RULES[form]
    check(r, layout, form, iters, None, seed=1)
    peak_gflops = cus * 4 * (flop / cycles) * MAX_CLOCK_HZ / 1e9
    mfmas_per_simd = r["work_per_launch"] / flop / (4 * cus)
    per_mfma = [l["clock_ghz"] * 1e9 * l["seconds"] / mfmas_per_simd
                for l in r["launches"]]
    print(form, "from LDS, rate:", r["rate"], "GFLOP/s of a peak of", peak_gflops,
          "clock_ghz:", r["clock_ghz"],
          "cycles per MFMA and SIMD:", [round(c, 3) for c in per_mfma])
    assert len(r["launches"]) == 8
    assert 0 < r["rate"] < peak_gflops
    for l in r["launches"]:
        assert 0 < l["rate"] < peak_gflops
    assert min(per_mfma) >= cycles * 0.95, per_mfma


def report_for(masks, form):
    tenants = [{"mask": masks["a50"]}, {"mask": masks["b50"]}]
    report = isolation_report(0, tenants, pairs=[("mfma", "mfma")], launches=8,
                              timeout=120.0, form=form, operands="lds")
    print("50 + 50, mfma/mfma from LDS,", form, ":", report)
    assert report.get("reason") != "child-failed", report
    return report


def check_split(t, solo):
    assert t["contended_launches"] >= 3, t
    for field in ("solo_clock_ghz", "contended_clock_ghz", "clock_ratio", "cycle_ratio"):
        assert t[field] > 0, (field, t)
    assert t["cycle_ratio"] * t["clock_ratio"] == pytest.approx(t["ratio"])
    assert t["clock_ratio"] == pytest.approx(
        t["contended_clock_ghz"] / t["solo_clock_ghz"])
    assert t["solo_rate"] == solo["rate"] and t["solo_clock_ghz"] == solo["clock_ghz"]


@pytest.mark.parametrize("form,spread", (("bf16", BF16_LDS_PAIR_SPREAD),
                                         ("mxfp4", MXFP4_LDS_PAIR_SPREAD)))
def test_two_processes_with_operands_from_lds(masks, form, spread):
    """One report for two 50-share tenants of one form, both reading their
    operands from LDS: alone (two children) and together (two more). The
    ratio and its split are the result (profiles/
    mfma_lds_cotenancy_results.md), not a bound; asserted are their sanity
    and that both tenants provably overlapped."""
    report = report_for(masks, form)
    assert report["ok"], report  # children exited 0, checksums right, overlap
    pair = report["pairs"]["mfma/mfma"]
    assert pair["ok"], pair
    for i, t in enumerate(pair["tenants"]):
        assert t["kind"] == "mfma" and t["form"] == form and t["operands"] == "lds"
        assert report["solo"][i]["mfma"]["form"] == form
        assert report["solo"][i]["mfma"]["operands"] == "lds"
        check_split(t, report["solo"][i]["mfma"])
        assert 0 < t["ratio"] <= 1 + half_width(spread), t
