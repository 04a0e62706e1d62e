"""The cache tenant on a real MI355X: it reads every byte of its working set
once per pass, stamps its launches sanely, reads faster than HBM can serve
while the working set fits the L2 and no faster than HBM once it does not,
and runs as one of two processes next to a 1 GiB streamer.

Every mask launched here comes from CardMaskPlan over the measured layout,
so it is a union of whole granules. If the layout does not come back
interleaved nothing masked is launched. Every child process has its own
timeout, and the first one that fails or times out ends the report it
belongs to: nothing further is started (agent/cotenancy.py).

Bands follow test_gpu_cotenancy.py: half-width max(0.1, 2 x observed
spread) around the value observed on an MI355X (profiles/
cache_cotenancy_results.md). The 8000 GB/s line is not observed but
derived: it is the HBM3E peak, which nothing served from HBM exceeds, while
the L2s together serve about 34.5 TB/s."""
from __future__ import annotations

import statistics

import pytest

from elastic_gpu_scheduler_amd.agent.cotenancy import cache_passes, isolation_report
from elastic_gpu_scheduler_amd.agent.cumask import CardMaskPlan, popcount

pytestmark = pytest.mark.gpu

SEED = 0x5EED
MIB = 1 << 20
GIB = 1 << 30
HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E peak; nothing read from HBM goes faster

# seconds / event_seconds at the default window (16 MiB x 1023 passes),
# unmasked: observed median and run-to-run spread.
STAMP_RATIO, STAMP_SPREAD = 0.99384, 0.00040
# spread of the cache tenant's contended / solo ratio beside a 1 GiB
# streamer, 50 + 50 shares, 12 MiB: the margin by which a contended tenant
# may appear faster than alone.
CACHE_PAIR_SPREAD = 0.042
# likewise for the streamer beside the cache tenant.
STREAM_PAIR_SPREAD = 0.021


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


@pytest.fixture(scope="module")
def expected(probe):
    """pattern_xor per buffer size and seed, computed once."""
    cache = {}

    def want(nbytes, seed=SEED):
        if (nbytes, seed) not in cache:
            cache[nbytes, seed] = probe.pattern_xor(seed, 0, nbytes // 8)
        return cache[nbytes, seed]

    return want


# One element, so that all but one workgroup have an empty chunk; one more
# than a whole step of four loads for 256 lanes; and a size that the grid
# does not divide, so that the chunks are unequal.
CACHE_SIZES = [16, 16 * (4 * 256 + 1), 3 * MIB + 16]


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "one-granule"])
@pytest.mark.parametrize("nbytes", CACHE_SIZES)
def test_cache_reads_every_byte_once_per_pass(probe, layout, masks, expected, nbytes,
                                              masked):
    """Tail, empty-chunk and single-element cases: meaningless as bandwidth."""
    mask = masks["tiny"] if masked else None
    for passes in (1, 3, 2):
        r = probe.cu_tenant_run(0, mask=mask, kind="cache", launches=2,
                                bytes=nbytes, passes=passes, seed=SEED)
        print(nbytes, "B", passes, "passes:", [l["seconds"] for l in r["launches"]])
        assert r["kind"] == "cache" and r["bytes"] == nbytes
        assert r["passes"] == (3 if passes == 2 else passes)  # even -> odd
        assert r["work_per_launch"] == nbytes * r["passes"]
        assert r["workgroups"] == 8 * layout["cus"]  # whatever the mask
        assert r["bytes_per_cu"] == pytest.approx(nbytes / layout["cus"])
        assert r["applied_mask"] == mask
        assert len(r["launches"]) == 2
        assert r["checksum"] == expected(nbytes), (nbytes, passes, masked)


def test_cache_rounds_bytes_down_to_sixteen(probe, expected):
    r = probe.cu_tenant_run(0, kind="cache", launches=1, bytes=16 * 77 + 9,
                            passes=1, seed=SEED)
    assert r["bytes"] == 16 * 77 and r["checksum"] == expected(16 * 77)
    r = probe.cu_tenant_run(0, kind="cache", launches=1, bytes=3, passes=1, seed=SEED)
    assert r["bytes"] == 16 and r["checksum"] == expected(16)


@pytest.fixture(scope="module")
def default_run(probe):
    """The default window, unmasked: 16 MiB x 1023 passes, 8 launches."""
    return probe.cu_tenant_run(0, kind="cache")


def test_cache_stamps_are_sane(default_run, expected):
    r = default_run
    runs = r["launches"]
    ratios = [l["seconds"] / l["event_seconds"] for l in runs]
    print("seconds:", [l["seconds"] for l in runs],
          "event_seconds:", [l["event_seconds"] for l in runs],
          "ratios:", [round(x, 4) for x in ratios], "rate:", r["rate"],
          "tick_hz:", r["tick_hz"], "workgroups:", r["workgroups"])
    assert (r["bytes"], r["passes"]) == (16 * MIB, 1023)
    assert r["checksum"] == expected(16 * MIB, seed=1)
    assert len(runs) == 8 and r["tick_hz"] > 0 and r["applied_mask"] is None
    for l in runs:
        assert l["t0"] < l["t1"]
        assert l["seconds"] == pytest.approx((l["t1"] - l["t0"]) / r["tick_hz"])
        assert l["seconds"] <= l["event_seconds"]
        assert l["rate"] == pytest.approx(r["work_per_launch"] / l["seconds"] / 1e9)
    for a, b in zip(runs, runs[1:]):
        assert a["t1"] <= b["t0"]
    assert r["rate"] == pytest.approx(statistics.median(l["rate"] for l in runs))
    assert abs(statistics.median(ratios) - STAMP_RATIO) <= half_width(STAMP_SPREAD), ratios


def test_it_is_a_cache_that_is_read(probe, default_run):
    """16 MiB is half the aggregate L2 and each workgroup's 8 KiB stays with
    one XCD, so the rate must lie above anything HBM can serve; 1 GiB is four
    Infinity Caches, so there it must lie below. Observed: 26.9 to 30.7 TB/s
    and 6.15 to 6.19 TB/s."""
    print("16 MiB:", default_run["rate"], [l["rate"] for l in default_run["launches"]])
    assert default_run["rate"] > HBM_PEAK_GBPS
    big = probe.cu_tenant_run(0, kind="cache", bytes=GIB, passes=7, launches=4)
    print("1 GiB:", big["rate"], [l["rate"] for l in big["launches"]])
    assert (big["bytes"], big["passes"]) == (GIB, 7)
    assert 0 < big["rate"] < HBM_PEAK_GBPS


CACHE_WINDOW = {"bytes": 12 * MIB, "passes": cache_passes(12 * MIB)}


@pytest.fixture(scope="module")
def beside_a_streamer(masks):
    """One report for two 50-share tenants: a 12 MiB cache tenant and the
    default 1 GiB x 127 streamer, alone (two children) and together (two
    more). The cache tenant's passes give its launch the bytes of a stream
    launch, so neither needs more launches than the probe allows."""
    report = isolation_report(
        0, [{"mask": masks["a50"]}, {"mask": masks["b50"]}],
        pairs=[("cache", "stream")], launches=8, timeout=120.0,
        windows={"cache": CACHE_WINDOW})
    print("50 + 50, cache/stream:", report)
    assert report.get("reason") != "child-failed", report
    return report


def test_two_processes_cache_beside_stream(beside_a_streamer):
    """The cache tenant's ratio is the result (profiles/
    cache_cotenancy_results.md), not a bound; asserted are its sanity, that
    both tenants provably overlapped, and on which side of the HBM peak each
    tenant's rates lie. Observed over four reports: the cache tenant keeps
    0.870 to 0.912 of its 19.4 TB/s, the streamer 0.964 to 0.985 of its 6.0."""
    report = beside_a_streamer
    assert report["ok"], report  # children exited 0, checksums right, overlap
    pair = report["pairs"]["cache/stream"]
    assert pair["ok"], pair
    cache, stream = pair["tenants"]
    assert (cache["kind"], stream["kind"]) == ("cache", "stream")
    for t, spread in ((cache, CACHE_PAIR_SPREAD), (stream, STREAM_PAIR_SPREAD)):
        assert t["contended_launches"] >= 3, t
        assert 0 < t["ratio"] <= 1 + half_width(spread), t
    assert 0 < stream["contended_rate"] < HBM_PEAK_GBPS, stream
    assert 0 < stream["solo_rate"] < HBM_PEAK_GBPS, stream
    assert cache["solo_rate"] == report["solo"][0]["cache"]["rate"]
    assert stream["solo_rate"] == report["solo"][1]["stream"]["rate"]
    # 12 MiB under a 50-share mask read 19.39 to 19.49 TB/s in all six solo
    # runs, and the sweep's 8 and 16 MiB 18.2 to 18.5: far above the HBM peak,
    # so alone it is the L2 that is read.
    assert cache["solo_rate"] > HBM_PEAK_GBPS, cache
