"""The decode tenants on pre-tiled weights (weights="tiled") on a real MI355X:
test_gpu_decode_cotenancy.py's own checks, shapes and bounds, run on the tiled
layout against the same closed form, which does not take the layout. Rates and
ratios are the result (profiles/decode_tiled_cotenancy_results.md), no bound."""
from __future__ import annotations

from types import SimpleNamespace

import pytest

from elastic_gpu_scheduler_amd.agent.cotenancy import isolation_report
from tests import test_gpu_decode_cotenancy as rows
from tests.test_gpu_decode_cotenancy import DISTANCE, FORMS, SHAPES, check, run
from tests.test_gpu_mxgemm_cotenancy import KEYS, SEED, layout, masks, probe  # noqa: F401

pytestmark = pytest.mark.gpu

# spread (max - min over five reports, 50 + 50 shares, default windows) of a
# tiled decode-mxfp4 tenant's and of the streamer's contended / solo ratio
# beside each other, the larger (profiles/decode_tiled_cotenancy_results.md).
TILED_PAIR_SPREAD = 0.0446  # (0.0197, 0.0446)


@pytest.fixture(scope="module")
def tiled(probe):
    """The probe, asked for tiled weights: a result must be the row-major one
    but for "weights" after load_bytes_per_launch, which is taken out."""
    def cu_tenant_run(*args, **window):
        r = probe.cu_tenant_run(*args, weights="tiled", **window)
        assert list(r)[KEYS.index("load_bytes_per_launch") + 1] == "weights"
        assert r.pop("weights") == "tiled"
        return r

    return SimpleNamespace(cu_tenant_run=cu_tenant_run)


@pytest.mark.parametrize("n,steps,passes", SHAPES)
@pytest.mark.parametrize("kind", FORMS)
def test_checksum_equals_the_closed_form_unmasked(tiled, kind, n, steps, passes):
    rows.test_checksum_equals_the_closed_form_unmasked(tiled, kind, n, steps, passes)


@pytest.mark.parametrize("n,steps,passes", ((384, DISTANCE + 1, 1), (128, 3, 1)))
@pytest.mark.parametrize("kind", FORMS)
def test_checksum_equals_the_closed_form_one_granule(tiled, masks, kind, n, steps, passes):
    rows.test_checksum_equals_the_closed_form_one_granule(tiled, masks, kind, n, steps, passes)


@pytest.mark.parametrize("kind", FORMS)
def test_both_layouts_give_one_checksum_and_rows_keeps_its_keys(probe, tiled, kind):
    a, b = (run(tiled, kind, 384, 3, 1, seed=seed) for seed in (SEED, SEED + 1))
    same = run(probe, kind, 384, 3, 1, seed=SEED, weights="rows")
    check(a, kind, 384, 3, 1, None)
    check(b, kind, 384, 3, 1, None, seed=SEED + 1)
    check(same, kind, 384, 3, 1, None)  # exactly today's keys
    assert a["checksum"] == same["checksum"] != b["checksum"]


@pytest.mark.parametrize("kind", FORMS)
def test_the_default_window_stays_below_the_form_s_mfma_peak(tiled, layout, kind):
    """The row-major window's derived bounds; the GB/s of weights is printed."""
    rows.test_the_default_window_stays_below_the_form_s_mfma_peak(tiled, layout, kind)


def test_two_processes_a_tiled_decode_tenant_beside_a_streamer(masks):
    """One report; the ratios are the result, asserted are sanity and overlap."""
    pair = ("decode-mxfp4", "stream")
    report = isolation_report(0, [{"mask": masks["a50"]}, {"mask": masks["b50"]}],
                              pairs=[pair], launches=8, timeout=120.0, weights="tiled")
    print("50 + 50, decode-mxfp4 tiled/stream:", report)
    assert report["ok"], report  # children exited 0, checksums right, overlap
    decode, stream = report["pairs"]["/".join(pair)]["tenants"]
    assert decode["weights"] == report["solo"][0][pair[0]]["weights"] == "tiled"
    assert "weights" not in stream and "weights" not in report["solo"][1]["stream"]
    assert decode["contended_launches"] >= 3 and stream["contended_launches"] >= 3
    assert decode["cycle_ratio"] * decode["clock_ratio"] == pytest.approx(decode["ratio"])
    for t in (decode, stream):
        assert 0 < t["ratio"] <= 1 + max(0.1, 2 * TILED_PAIR_SPREAD), t
