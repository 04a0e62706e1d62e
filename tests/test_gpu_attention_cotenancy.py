"""The attention tenant (a causal flash-attention forward pass in bf16: K and
V global memory -> LDS, S^T = K Q^T and O^T = V^T P^T on the matrix cores, the
softmax online in base 2) on a real MI355X: every element of its output
against float64 at the diagonal tile alone, at the ring's prologue and
epilogue, at an odd tile count, over several heads and passes and in the
steady state, unmasked and under the smallest mask; the probe's own sampled
reference agrees; the default window stays below the MFMA peak; and an
attention tenant runs beside a streamer as two processes.

Fixtures, masks and children are test_gpu_mxgemm_cotenancy.py's. The data rule
is agent/cotenancy.py's attention_operands(), the tolerance its derived
ATTENTION_TOLERANCE. How large rate and ratios are is the result
(profiles/attention_cotenancy_results.md), not a bound."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from elastic_gpu_scheduler_amd.agent.cotenancy import (ATTENTION_TOLERANCE, attention_operands,
                                                       isolation_report)
from tests.test_gpu_gemm_cotenancy import MFMA_CYCLES, MFMA_FLOP  # v_mfma_f32_32x32x16_bf16
from tests.test_gpu_mxgemm_cotenancy import (  # noqa: F401  (fixtures)
    LAUNCH_KEYS, MAX_CLOCK_HZ, SEED, layout, masks, probe)

pytestmark = pytest.mark.gpu

KEYS = ["kind", "applied_mask", "tick_hz", "workgroups", "seq", "heads", "head_dim", "bytes",
        "out_bytes", "passes", "max_error", "checked_rows", "load_bytes_per_launch",
        "work_per_launch", "launches", "rate", "clock_ghz"]
# (iters, heads): the diagonal tile alone; the first full tile plus prologue
# and epilogue of the ring; an odd ring count and a second head; counts the
# XCDs do not divide; the steady state.
SHAPES = ((1, 1), (2, 1), (3, 2), (5, 3), (8, 1))
# spread (max - min over five reports, 50 + 50 shares, default windows) of an
# attention tenant's contended / solo ratio beside another one
# (profiles/attention_cotenancy_results.md).
ATTENTION_PAIR_SPREAD = 0.0055  # (0.0055, 0.0055)


@functools.lru_cache(maxsize=None)
def reference(seed, head, seq):
    """float64 causal softmax(Q K^T / sqrt(128)) V of one head, and its V."""
    q, k, v = (np.array(x) for x in attention_operands(seed, head, seq))
    s = q @ k.T / np.sqrt(128.0)
    s[np.triu_indices(seq, 1)] = -np.inf
    p = np.exp(s - s.max(axis=1, keepdims=True))
    return (p / p.sum(axis=1, keepdims=True)) @ v, v


def output(probe, iters, heads, seed=SEED, **more):
    r = probe.attention_output(0, iters=iters, bytes=768 * 128 * iters * heads, seed=seed, **more)
    assert (r["seq"], r["heads"]) == (128 * iters, heads)
    bits = np.frombuffer(r["output"], dtype="<u2").astype(np.uint32) << 16
    return bits.view(np.float32).astype(np.float64).reshape(heads, 128 * iters, 128)


def errors(got, seed):
    heads, seq, _ = got.shape
    for head in range(heads):
        want, v = reference(seed, head, seq)
        assert (got[head, 0] == v[0]).all(), head  # row 0 attends to one key
        yield np.abs(got[head] - want).max()


@pytest.mark.parametrize("iters,heads", SHAPES)
def test_every_element_equals_the_float64_reference(probe, iters, heads):
    worst = max(errors(output(probe, iters, heads), SEED))
    print("iters", iters, "heads", heads, "max |O - reference|:", worst)
    assert worst <= ATTENTION_TOLERANCE


def test_two_seeds_give_two_outputs(probe):
    a, b = (output(probe, 3, 2, seed=seed) for seed in (SEED, SEED + 1))
    assert max(errors(a, SEED)) <= ATTENTION_TOLERANCE
    assert max(errors(b, SEED + 1)) <= ATTENTION_TOLERANCE
    assert (a != b).any()


def check(r, iters, heads, passes, mask, launches=2):
    seq = 128 * iters
    assert list(r) == KEYS
    assert len(r["launches"]) == launches
    assert all(list(l) == LAUNCH_KEYS for l in r["launches"])
    assert (r["kind"], r["seq"], r["heads"], r["head_dim"], r["passes"]) == (
        "attention", seq, heads, 128, passes)
    assert r["bytes"] == 768 * seq * heads and r["out_bytes"] == 256 * seq * heads * passes
    assert r["workgroups"] == passes * heads * iters
    assert r["work_per_launch"] == passes * heads * 4 * 128 * seq * (seq + 1) // 2
    assert r["load_bytes_per_launch"] == passes * heads * 32768 * iters * (iters + 2)
    assert r["applied_mask"] == mask
    assert r["checked_rows"] == min(256, passes * heads * seq)
    assert r["max_error"] <= ATTENTION_TOLERANCE, r["max_error"]


@pytest.mark.parametrize("tiny", (False, True))
@pytest.mark.parametrize("passes", (1, 3))
@pytest.mark.parametrize("iters,heads", SHAPES)
def test_the_tenant_run_reports_its_shape_and_its_error(probe, masks, iters, heads, passes, tiny):
    mask = masks["tiny"] if tiny else None
    r = probe.cu_tenant_run(0, kind="attention", launches=2, iters=iters, passes=passes,
                            bytes=768 * 128 * iters * heads, seed=SEED, mask=mask)
    check(r, iters, heads, passes, mask)


def test_the_default_window_stays_below_the_mfma_peak(probe, layout):
    """Derived, none observed: the rate stays below the bf16 MFMA peak at 2.4
    GHz. Rate, clock and cycles per MFMA and SIMD are printed, not bounded."""
    r, cus = probe.cu_tenant_run(0, kind="attention"), layout["cus"]
    check(r, 64, 64, r["passes"], None, launches=8)
    peak_gflops = cus * 4 * (MFMA_FLOP / MFMA_CYCLES) * MAX_CLOCK_HZ / 1e9
    # issued: 32 MFMAs per wave and tile, 2 (t + 1) tiles on query tile t < 64
    mfmas_per_simd = r["passes"] * r["heads"] * 64 * 65 * 32 * 4 / (4 * cus)
    per_mfma = [l["clock_ghz"] * 1e9 * l["seconds"] / mfmas_per_simd for l in r["launches"]]
    print("attention passes:", r["passes"], "rate:", r["rate"], "GFLOP/s of a peak of",
          peak_gflops, "clock_ghz:", r["clock_ghz"], "launch seconds:",
          [l["seconds"] for l in r["launches"]], "cycles per MFMA and SIMD:",
          [round(c, 2) for c in per_mfma], "max_error:", r["max_error"])
    assert 0 < r["rate"] < peak_gflops
    assert all(0 < l["rate"] < peak_gflops for l in r["launches"])


def test_two_processes_an_attention_tenant_beside_a_streamer(masks):
    """One report for a 50-share attention tenant and a 50-share streamer:
    alone and together. The ratios are the result; asserted are their sanity
    and that both provably overlapped."""
    pair = ("attention", "stream")
    report = isolation_report(0, [{"mask": masks["a50"]}, {"mask": masks["b50"]}],
                              pairs=[pair], launches=8, timeout=120.0)
    print("50 + 50, attention/stream:", report)
    assert report["ok"], report  # children exited 0, output and checksum right, overlap
    attention, stream = report["pairs"]["/".join(pair)]["tenants"]
    assert attention["contended_launches"] >= 3 and stream["contended_launches"] >= 3
    assert attention["cycle_ratio"] * attention["clock_ratio"] == pytest.approx(
        attention["ratio"])
    for t in (attention, stream):
        assert 0 < t["ratio"] <= 1 + max(0.1, 2 * ATTENTION_PAIR_SPREAD), t
