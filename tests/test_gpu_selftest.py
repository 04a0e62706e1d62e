"""Deep card self-test on a real MI355X: the HBM pattern test, per-XCD read
bandwidth and the MFMA check, at the smallest shapes at which each kernel can
still go wrong, plus the agent's self_test() on a healthy card.

Small buffers here are served from cache; that is what a kernel-logic test
wants. Only the agent defaults (>= 1 GiB) say anything about HBM cells."""
from __future__ import annotations

import pytest

pytestmark = pytest.mark.gpu

MiB = 1024**2
GiB = 1024**3
SEED = 0x0123456789ABCDEF


@pytest.fixture(scope="module")
def probe():
    from elastic_gpu_scheduler_amd._native import gpuprobe

    p = gpuprobe()  # raises loudly if the HIP extension is missing
    if p.device_count() == 0:
        pytest.fail("gpu-marked test ran but no HIP device is visible")
    return p


@pytest.fixture(scope="module")
def grid(probe):
    return 4 * probe.device_info(0)["multi_processor_count"]


# --- HBM pattern -----------------------------------------------------------

@pytest.mark.parametrize("nbytes", [16, 16 * (64 * 3 + 1), MiB + 16])
def test_pattern_clean(probe, nbytes):
    r = probe.hbm_pattern_test(0, nbytes, SEED)
    assert r["bytes"] == nbytes
    assert r["mismatches"] == [0, 0] and r["records"] == []
    assert r["seconds"] > 0


def test_pattern_rounds_down_to_16(probe):
    r = probe.hbm_pattern_test(0, 16 * 5 + 15, SEED)
    assert r["bytes"] == 80 and r["mismatches"] == [0, 0]


def test_pattern_reports_injected_words(probe):
    nbytes = MiB + 16
    last = nbytes // 8 - 1
    injected = [
        (0, 0, 0xFFFFFFFFFFFFFFFF),      # first word, every bit
        (0, last // 2, 1 << 17),         # a middle word, one bit
        (0, last, 0x8000000000000001),   # last word
        (1, 12345, 1 << 63),             # complement pass
    ]
    r = probe.hbm_pattern_test(0, nbytes, SEED, corrupt=injected)
    assert r["mismatches"] == [3, 1]
    assert r["records"] == sorted(injected)


def test_pattern_record_list_is_capped(probe):
    injected = [(0, 3 * i + 1, 1 << i) for i in range(20)]
    r = probe.hbm_pattern_test(0, MiB, SEED, corrupt=injected)
    assert r["mismatches"] == [20, 0]
    assert len(r["records"]) == 16
    assert set(r["records"]) <= set(injected)


def test_pattern_rejects_bad_corruption(probe):
    with pytest.raises(ValueError):
        probe.hbm_pattern_test(0, 64, SEED, corrupt=[(0, 8, 1)])
    with pytest.raises(ValueError):
        probe.hbm_pattern_test(0, 64, SEED, corrupt=[(2, 0, 1)])
    with pytest.raises(RuntimeError):
        probe.hbm_pattern_test(10_000, 64, SEED)


def test_pattern_beyond_4gib(probe):
    """Index arithmetic past 2^32 bytes: only the last word of a
    4 GiB + 4096 buffer is corrupted, and only it may be reported."""
    nbytes = 4 * GiB + 4096
    last = nbytes // 8 - 1
    r = probe.hbm_pattern_test(0, nbytes, SEED, corrupt=[(0, last, 1 << 5)])
    if "skipped" in r:
        pytest.skip(f"free-memory check declined: {r['free_bytes']} bytes free")
    assert r["bytes"] == nbytes
    assert r["mismatches"] == [1, 0]
    assert r["records"] == [(0, last, 1 << 5)]


# --- per-XCD bandwidth -----------------------------------------------------

def test_xcd_bandwidth_reads_each_slice_once(probe):
    entries = probe.xcd_bandwidth(0, slice_mib=1, chunk_kib=64, iters=2)
    print("xcd_bandwidth:", entries)
    assert 1 <= len(entries) <= 8
    ids = [e["xcc"] for e in entries]
    assert len(set(ids)) == len(ids) and all(0 <= x <= 7 for x in ids)
    words = MiB // 8
    for e in entries:
        assert e["chunks"] == 16 and e["bytes"] == MiB
        assert e["workgroups"] > 0
        assert e["checksum"] == probe.pattern_xor(
            probe.XCD_PATTERN_SEED, e["xcc"] * words, words)
        assert e["stable"] is True
        assert e["gbps"] > 0 and e["seconds"] > 0


def test_xcd_bandwidth_other_seed_and_chunking(probe):
    entries = probe.xcd_bandwidth(0, slice_mib=2, chunk_kib=4, iters=1, seed=SEED)
    words = 2 * MiB // 8
    assert entries
    for e in entries:
        assert e["chunks"] == 512
        assert e["checksum"] == probe.pattern_xor(SEED, e["xcc"] * words, words)
    with pytest.raises(ValueError):
        probe.xcd_bandwidth(0, slice_mib=1, chunk_kib=6, iters=1)
    with pytest.raises(ValueError):
        probe.xcd_bandwidth(0, slice_mib=1, chunk_kib=2048, iters=1)


# --- MFMA ------------------------------------------------------------------

@pytest.mark.parametrize("iters", [4, 1024])
def test_mfma_matches_vector_alu(probe, grid, iters):
    entries = probe.mfma_selftest(0, iters=iters)
    print("mfma_selftest:", entries)
    assert entries
    assert all(e["mismatched_elements"] == 0 for e in entries), entries
    assert sum(e["workgroups"] for e in entries) == grid
    ids = [e["xcc"] for e in entries]
    assert len(set(ids)) == len(ids)


def test_mfma_negative_control(probe, grid):
    entries = probe.mfma_selftest(0, iters=4, perturb_wg=5)
    bad = [e for e in entries if e["mismatched_elements"]]
    assert len(bad) == 1 and bad[0]["mismatched_elements"] == 32, entries
    assert sum(e["workgroups"] for e in entries) == grid


# --- agent -----------------------------------------------------------------

def test_agent_self_test_healthy_card(probe):
    from elastic_gpu_scheduler_amd.agent.agent import NodeAgent

    report = NodeAgent("local").self_test(pattern_mib=64, slice_mib=8,
                                          mfma_iters=16)
    assert len(report) == probe.device_count()
    for r in report:
        assert r["healthy"] and r["reasons"] == [], r
        assert r["pattern"]["bytes"] == 64 * MiB
        assert r["pattern"]["mismatches"] == [0, 0]
        assert all(e["chunks"] == e["expected_chunks"] == 32 for e in r["xcd"])
        assert r["mfma"] and r["hbm_gbps"] > 1000.0
