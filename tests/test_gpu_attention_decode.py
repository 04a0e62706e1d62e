"""The attention-decode tenant (16 query rows against a head's K and V streamed
once, split along the keys) on a real MI355X: every element of its output
against float64; the probe's own sampled reference agrees; the default window
stays below the MFMA and the HBM peak; and it runs beside a streamer as two
processes. Fixtures, masks and children are test_gpu_mxgemm_cotenancy.py's; how
large rate and ratios are is the result
(profiles/attention_decode_cotenancy_results.md), not a bound."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from elastic_gpu_scheduler_amd.agent.cotenancy import (ATTENTION_TOLERANCE,
                                                       attention_decode_length,
                                                       attention_decode_shape,
                                                       attention_operands, isolation_report)
from tests.test_gpu_chase_cotenancy import HBM_PEAK_GBPS
from tests.test_gpu_mxgemm_cotenancy import (  # noqa: F401  (fixtures)
    LAUNCH_KEYS, MAX_CLOCK_HZ, SEED, layout, masks, probe)

pytestmark = pytest.mark.gpu

KIND = "attention-decode"
KEYS = ["kind", "applied_mask", "tick_hz", "workgroups", "seq", "heads", "head_dim", "queries",
        "splits", "bytes", "out_bytes", "passes", "max_error", "checked_rows",
        "load_bytes_per_launch", "work_per_launch", "launches", "rate", "clock_ghz"]
# (iters, heads): one tile per wave, full length; lengths 128, 91, 54 and 17,
# partial tiles and waves with no key; a tile count the four waves do not
# divide; eight tiles per wave, the ring in its steady state and at its wrap;
# two splits of 5 and 4 units, the second ragged; three splits of 6, 6 and 5.
SHAPES = ((1, 1), (1, 4), (3, 2), (8, 1), (9, 2), (17, 3))
MFMA_FLOP, MFMA_CYCLES = 2 * 16 * 16 * 32, 8  # v_mfma_f32_16x16x32_bf16
# spread (max - min over five reports, 50 + 50 shares, default windows) of an
# attention-decode tenant's contended / solo ratio beside another one: not
# measured yet (profiles/attention_decode_cotenancy_results.md), so the bound
# below is its floor of 0.1.
ATTENTION_DECODE_PAIR_SPREAD = 0.0


def window_bytes(iters, heads):
    return heads * (512 * 128 * iters + 4096)


@functools.lru_cache(maxsize=None)
def reference(seed, head, seq):
    """float64 softmax(Q K[:len]^T / sqrt(128)) V[:len] of one head's 16 rows,
    its V and its length."""
    n = attention_decode_length(head, seq)
    q, k, v = (np.array(x) for x in attention_operands(seed, head, seq))
    s = q[:16] @ k[:n].T / np.sqrt(128.0)
    p = np.exp(s - s.max(axis=1, keepdims=True))
    return (p / p.sum(axis=1, keepdims=True)) @ v[:n], v, n


def output(probe, iters, heads, seed=SEED):
    r = probe.attention_output(0, iters=iters, bytes=window_bytes(iters, heads), seed=seed,
                               kind=KIND)
    assert (r["seq"], r["heads"], r["queries"], r["splits"]) == (
        128 * iters, heads, 16, attention_decode_shape(window_bytes(iters, heads), iters)[3])
    bits = np.frombuffer(r["output"], dtype="<u2").astype(np.uint32) << 16
    return bits.view(np.float32).astype(np.float64).reshape(heads, 16, 128)


def worst(got, seed, seq):
    return max(np.abs(got[head] - reference(seed, head, seq)[0]).max()
               for head in range(got.shape[0]))


@pytest.mark.parametrize("iters,heads", SHAPES)
def test_every_element_equals_the_float64_reference(probe, iters, heads):
    error = worst(output(probe, iters, heads), SEED, 128 * iters)
    print("iters", iters, "heads", heads, "max |O - reference|:", error)
    assert error <= ATTENTION_TOLERANCE


def test_a_head_of_one_key_returns_that_key_s_value(probe):
    want, v, n = reference(SEED, 83, 128)
    got = output(probe, 1, 84)[83]
    assert n == 1 and (got == v[0]).all() and (want == v[0]).all()


def test_two_seeds_give_two_outputs(probe):
    a, b = (output(probe, 9, 2, seed=seed) for seed in (SEED, SEED + 1))
    assert worst(a, SEED, 1152) <= ATTENTION_TOLERANCE
    assert worst(b, SEED + 1, 1152) <= ATTENTION_TOLERANCE
    assert (a != b).any()


def check(r, iters, heads, passes, mask, launches=2):
    seq, splits = 128 * iters, attention_decode_shape(window_bytes(iters, heads), iters)[3]
    live = sum(attention_decode_length(h, seq) for h in range(heads))
    assert list(r) == KEYS
    assert len(r["launches"]) == launches
    assert all(list(l) == LAUNCH_KEYS for l in r["launches"])
    assert (r["kind"], r["seq"], r["heads"], r["head_dim"], r["queries"], r["splits"],
            r["passes"]) == (KIND, seq, heads, 128, 16, splits, passes)
    assert r["bytes"] == window_bytes(iters, heads) and r["out_bytes"] == 4096 * heads * passes
    assert r["workgroups"] == passes * heads * splits
    assert r["work_per_launch"] == passes * 4 * 128 * 16 * live
    assert r["load_bytes_per_launch"] == passes * (512 * live + 4096 * heads * splits)
    assert r["applied_mask"] == mask
    assert r["checked_rows"] == min(256, passes * heads * 16)
    assert r["max_error"] <= ATTENTION_TOLERANCE, r["max_error"]


@pytest.mark.parametrize("tiny", (False, True))
@pytest.mark.parametrize("passes", (1, 3))
@pytest.mark.parametrize("iters,heads", SHAPES + ((3, 700), (9, 700)))
def test_the_tenant_run_reports_its_shape_and_its_error(probe, masks, iters, heads, passes, tiny):
    """(3, 700) and (9, 700), one split and two uneven ones of 5 and 4 units,
    are too large for the Python reference: the probe's sampled one holds."""
    mask = masks["tiny"] if tiny else None
    r = probe.cu_tenant_run(0, kind=KIND, launches=2, iters=iters, passes=passes,
                            bytes=window_bytes(iters, heads), seed=SEED, mask=mask)
    check(r, iters, heads, passes, mask)


def test_the_default_window_stays_below_the_peaks(probe, layout):
    """Derived bounds, none observed; TB/s, clock and seconds are printed."""
    r, cus = probe.cu_tenant_run(0, kind=KIND), layout["cus"]
    check(r, 64, 256, r["passes"], None, launches=8)
    peak_gflops = cus * 4 * (MFMA_FLOP / MFMA_CYCLES) * MAX_CLOCK_HZ / 1e9
    gbps = [r["load_bytes_per_launch"] / l["seconds"] / 1e9 for l in r["launches"]]
    print("attention-decode passes:", r["passes"], "rate:", r["rate"], "GFLOP/s of a peak of",
          peak_gflops, "TB/s:", [round(x / 1e3, 3) for x in gbps], "clock_ghz:", r["clock_ghz"],
          "launch seconds:", [l["seconds"] for l in r["launches"]], "max_error:", r["max_error"])
    assert 0 < r["rate"] < peak_gflops
    assert all(0 < x < HBM_PEAK_GBPS for x in gbps)


def test_two_processes_an_attention_decode_tenant_beside_a_streamer(masks):
    """One report, 50 + 50 shares: the ratios' sanity and a proven overlap."""
    pair = (KIND, "stream")
    report = isolation_report(0, [{"mask": masks["a50"]}, {"mask": masks["b50"]}],
                              pairs=[pair], launches=8, timeout=120.0)
    print("50 + 50, attention-decode/stream:", report)
    assert report["ok"], report  # children exited 0, output and checksum right, overlap
    decode, stream = report["pairs"]["/".join(pair)]["tenants"]
    assert decode["contended_launches"] >= 3 and stream["contended_launches"] >= 3
    assert decode["cycle_ratio"] * decode["clock_ratio"] == pytest.approx(decode["ratio"])
    for t in (decode, stream):
        assert 0 < t["ratio"] <= 1 + max(0.1, 2 * ATTENTION_DECODE_PAIR_SPREAD), t
