"""The chase tenant on a real MI355X: every wave ends where the closed form
says, byte offsets past 4 GiB are 64-bit, its launches are stamped sanely,
its time per hop rises with each level of the hierarchy that its working set
no longer fits, and it runs as one of two processes next to a 1 GiB
streamer.

Every mask launched here comes from CardMaskPlan over the measured layout,
so it is a union of whole granules. If the layout does not come back
interleaved nothing masked is launched. Every child process has its own
timeout, and the first one that fails or times out ends the report it
belongs to: nothing further is started (agent/cotenancy.py).

The oracle is agent/cotenancy.py's chase_stride and chase_checksum, pure
Python and closed form, themselves checked against a brute-force walk in
test_chase_cotenancy_cpu.py. Bands follow test_gpu_cotenancy.py: half-width
max(0.1, 2 x observed spread) around the value observed on an MI355X
(profiles/chase_cotenancy_results.md). The ordering of the three latencies
and the 8000 GB/s line are not observed but derived."""
from __future__ import annotations

import statistics

import pytest

from elastic_gpu_scheduler_amd.agent.cotenancy import (chase_checksum, chase_stride,
                                                       isolation_report)
from elastic_gpu_scheduler_amd.agent.cumask import CardMaskPlan, popcount

pytestmark = pytest.mark.gpu

SEED = 0x5EED
MIB = 1 << 20
GIB = 1 << 30
HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E peak; nothing read from HBM goes faster

# seconds / event_seconds at the default window (1 GiB x 65536 hops),
# unmasked: observed median and run-to-run spread (max - min of the
# per-run medians) over five runs.
STAMP_RATIO, STAMP_SPREAD = 0.99984, 0.00002
# spread (max - min over five reports) of the chase tenant's contended / solo
# ratio beside a 1 GiB streamer, 50 + 50 shares, 1 GiB: the margin by which a
# contended tenant may appear faster than alone.
CHASE_PAIR_SPREAD = 0.004
# likewise for the streamer beside the chase tenant.
STREAM_PAIR_SPREAD = 0.018


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


# A self-loop; fewer nodes than waves, so that several waves start on one
# node; a prime, which the wave count does not divide; one more than a power
# of two; and 24577 nodes, three quarters of one XCD's L2, where the starts
# are unequally spaced.
CHASE_SIZES = [128, 128 * 3, 128 * 1021, 128 * 4097, 3 * MIB + 128]


def check(r, layout, nbytes, iters, mask):
    nodes = nbytes // 128
    assert r["kind"] == "chase" and r["bytes"] == nbytes and r["nodes"] == nodes
    assert r["stride"] == chase_stride(nodes)
    assert r["iters"] == iters and "passes" not in r
    assert r["workgroups"] == layout["cus"]  # whatever the mask
    assert r["work_per_launch"] == 4 * layout["cus"] * iters
    assert r["applied_mask"] == mask
    assert r["checksum"] == chase_checksum(nbytes, r["workgroups"], iters, SEED), (
        nbytes, iters, mask)


@pytest.mark.parametrize("nbytes", CHASE_SIZES)
def test_chase_ends_where_the_closed_form_says_unmasked(probe, layout, nbytes):
    """Self-loop, shared-start and odd-size cases: meaningless as latency."""
    for iters in (1, 2, 4099):
        r = probe.cu_tenant_run(0, kind="chase", launches=2, bytes=nbytes,
                                iters=iters, seed=SEED)
        print(nbytes, "B", iters, "hops:", [l["seconds"] for l in r["launches"]])
        assert len(r["launches"]) == 2
        check(r, layout, nbytes, iters, None)


@pytest.mark.parametrize("nbytes", CHASE_SIZES)
def test_chase_ends_where_the_closed_form_says_one_granule(probe, layout, masks, nbytes):
    """The same under the smallest mask, where workgroups queue for the CUs."""
    for iters in (1, 2, 4099):
        r = probe.cu_tenant_run(0, mask=masks["tiny"], kind="chase", launches=2,
                                bytes=nbytes, iters=iters, seed=SEED)
        print(nbytes, "B", iters, "hops:", [l["seconds"] for l in r["launches"]])
        assert len(r["launches"]) == 2
        check(r, layout, nbytes, iters, masks["tiny"])


def test_chase_rounds_bytes_down_to_a_line_and_defaults_iters(probe, layout):
    r = probe.cu_tenant_run(0, kind="chase", launches=1, bytes=128 * 77 + 9,
                            iters=3, seed=SEED)
    check(r, layout, 128 * 77, 3, None)
    r = probe.cu_tenant_run(0, kind="chase", launches=1, bytes=3, iters=3, seed=SEED)
    check(r, layout, 128, 3, None)
    r = probe.cu_tenant_run(0, kind="chase", launches=1, bytes=128 * 77, iters=0,
                            seed=SEED)
    check(r, layout, 128 * 77, 65536, None)


def test_chase_byte_offsets_are_64_bit(probe, layout):
    """4 GiB and five lines: the smallest buffer in which a 32-bit byte
    offset wraps. The waves' starts are spread over the whole buffer, so the
    nodes above 4 GiB are read at the first hop."""
    nbytes = 4 * GIB + 128 * 5
    r = probe.cu_tenant_run(0, kind="chase", launches=1, bytes=nbytes, iters=257,
                            seed=SEED)
    if "skipped" in r:
        pytest.skip(f"too little free memory for a 4 GiB buffer: {r}")
    check(r, layout, nbytes, 257, None)


@pytest.fixture(scope="module")
def default_run(probe):
    """The default window, unmasked: 1 GiB x 65536 hops, 8 launches."""
    return probe.cu_tenant_run(0, kind="chase")


def test_chase_stamps_are_sane(default_run, layout):
    r = default_run
    runs = r["launches"]
    ratios = [l["seconds"] / l["event_seconds"] for l in runs]
    print("seconds:", [l["seconds"] for l in runs],
          "event_seconds:", [l["event_seconds"] for l in runs],
          "ratios:", [round(x, 4) for x in ratios], "rate:", r["rate"],
          "ns_per_hop:", r["ns_per_hop"],
          "tick_hz:", r["tick_hz"], "workgroups:", r["workgroups"])
    assert (r["bytes"], r["iters"]) == (GIB, 65536)
    assert r["checksum"] == chase_checksum(GIB, layout["cus"], 65536, 1)
    assert len(runs) == 8 and r["tick_hz"] > 0 and r["applied_mask"] is None
    for l in runs:
        assert l["t0"] < l["t1"]
        assert l["seconds"] == pytest.approx((l["t1"] - l["t0"]) / r["tick_hz"])
        assert l["seconds"] <= l["event_seconds"]
        assert l["rate"] == pytest.approx(r["work_per_launch"] / l["seconds"] / 1e9)
    for a, b in zip(runs, runs[1:]):
        assert a["t1"] <= b["t0"]
    assert r["rate"] == pytest.approx(statistics.median(l["rate"] for l in runs))
    assert r["ns_per_hop"] == pytest.approx(
        statistics.median(l["seconds"] for l in runs) * 1e9 / r["iters"])
    assert abs(statistics.median(ratios) - STAMP_RATIO) <= half_width(STAMP_SPREAD), ratios


def test_it_is_latency_that_is_measured(probe, default_run):
    """Every XCD walks the whole buffer: 2 MiB fits one XCD's 4 MiB L2, 64
    MiB fits only the 256 MiB Infinity Cache, 1 GiB fits neither. On an idle
    chip one lane's dependent load takes about 180 to 225 cycles from the L2,
    545 from the Infinity Cache and 900 from HBM, levels at least 1.6 x
    apart, so the time per hop must rise strictly from each size to the
    next. How long a hop takes is a result (profiles/
    chase_cotenancy_results.md), not asserted."""
    small = probe.cu_tenant_run(0, kind="chase", bytes=2 * MIB, launches=4)
    middle = probe.cu_tenant_run(0, kind="chase", bytes=64 * MIB, launches=4)
    for r, size in ((small, 2 * MIB), (middle, 64 * MIB)):
        assert (r["bytes"], r["iters"]) == (size, 65536)
        assert r["checksum"] == chase_checksum(size, r["workgroups"], 65536, 1)
    print("ns per hop, 2 MiB:", small["ns_per_hop"], "64 MiB:", middle["ns_per_hop"],
          "1 GiB:", default_run["ns_per_hop"])
    assert 0 < small["ns_per_hop"] < middle["ns_per_hop"] < default_run["ns_per_hop"]


@pytest.fixture(scope="module")
def beside_a_streamer(masks):
    """One report for two 50-share tenants: a 1 GiB chase tenant and the
    default 1 GiB x 127 streamer, alone (two children) and together (two
    more)."""
    report = isolation_report(
        0, [{"mask": masks["a50"]}, {"mask": masks["b50"]}],
        pairs=[("chase", "stream")], launches=8, timeout=120.0,
        windows={"chase": {"bytes": 1 << 30}})
    print("50 + 50, chase/stream:", report)
    assert report.get("reason") != "child-failed", report
    return report


def test_two_processes_chase_beside_stream(beside_a_streamer):
    """The chase tenant's ratio is the result (profiles/
    chase_cotenancy_results.md), not a bound; asserted are its sanity, that
    both tenants provably overlapped, and that the streamer's rates lie
    below the HBM peak."""
    report = beside_a_streamer
    assert report["ok"], report  # children exited 0, checksums right, overlap
    pair = report["pairs"]["chase/stream"]
    assert pair["ok"], pair
    chase, stream = pair["tenants"]
    assert (chase["kind"], stream["kind"]) == ("chase", "stream")
    for t, spread in ((chase, CHASE_PAIR_SPREAD), (stream, STREAM_PAIR_SPREAD)):
        assert t["contended_launches"] >= 3, t
        assert 0 < t["ratio"] <= 1 + half_width(spread), t
    assert 0 < stream["contended_rate"] < HBM_PEAK_GBPS, stream
    assert 0 < stream["solo_rate"] < HBM_PEAK_GBPS, stream
    assert chase["solo_rate"] == report["solo"][0]["chase"]["rate"]
    assert stream["solo_rate"] == report["solo"][1]["stream"]["rate"]
    assert report["solo"][0]["chase"]["ns_per_hop"] > 0
