"""The gemm tenant without a GPU: its oracle against a brute-force product,
the shape rule, and what run_pair and isolation_report accept and refuse.
The fake children are test_mfma_forms_cpu's."""
from __future__ import annotations

import numpy as np
import pytest

from elastic_gpu_scheduler_amd.agent import cotenancy
from elastic_gpu_scheduler_amd.agent.cotenancy import (gemm_checksum, gemm_shape,
                                                       isolation_report, run_pair)
from tests.test_mfma_forms_cpu import TENANTS, FakeChild, Spawner, flag

SEED = 0x5EED


@pytest.mark.parametrize("m,n,k,passes", ((128, 128, 64, 1), (256, 256, 128, 3),
                                          (384, 384, 320, 2)))
def test_gemm_checksum_equals_the_brute_force_product(m, n, k, passes):
    key = cotenancy._mix32(SEED ^ 0x47454D4D)
    a = np.array([[cotenancy._mix32(key ^ (i % 192) << 8 ^ kk % 96 ^ 0xA00000) % 31 - 15
                   for kk in range(k)] for i in range(m)], dtype=np.int64)
    b = np.array([[cotenancy._mix32(key ^ (kk % 96) << 8 ^ j % 192 ^ 0xB00000) % 31 - 15
                   for kk in range(k)] for j in range(n)], dtype=np.int64)
    c = a @ b.T
    assert np.abs(c).max() < 1 << 23  # exact in f32
    one = int((c * np.outer(np.arange(1, m + 1), np.arange(1, n + 1))).sum())
    want = sum((1 + p) * one for p in range(passes)) % (1 << 64)
    assert gemm_checksum(m, n, k, passes, SEED) == want
    assert gemm_checksum(m, n, k, passes, SEED + 1) != want


@pytest.mark.parametrize("nbytes,iters,side,k", (
    (0, 0, 8192, 4096), (0, 1, 32768, 64), (0, 3, 32768, 192), (0, 10**6, 1024, 32768),
    (1, 0, 128, 4096), (1, 1, 128, 64), (1, 3, 128, 192), (1, 10**6, 128, 32768),
    (294912, 0, 128, 4096), (294912, 1, 1152, 64), (294912, 3, 384, 192),
    (294912, 10**6, 128, 32768),
    (1 << 40, 0, 32768, 4096), (1 << 40, 1, 32768, 64), (1 << 40, 3, 32768, 192),
    (1 << 40, 10**6, 32768, 32768)))
def test_gemm_shape_states_the_clamps(nbytes, iters, side, k):
    assert gemm_shape(nbytes, iters) == (side, side, k)


def child(n, argv, env):
    """A gemm child as the probe reports it, its clock 2.0 alone and 1.5
    from the third child on, which are the pair's."""
    m, _, k = gemm_shape(int(flag(argv, "--bytes")), int(flag(argv, "--iters")))
    passes, clock = int(flag(argv, "--passes")) or 16, 2.0 if n < 2 else 1.5
    launches = [{"t0": 1000 * i, "t1": 1000 * i + 999, "seconds": 999e-8, "rate": clock,
                 "clock_ghz": clock} for i in range(int(flag(argv, "--launches")))]
    return FakeChild(argv, env, {
        "kind": "gemm", "workgroups": (m // 128) ** 2 * passes, "m": m, "n": m, "k": k,
        "passes": passes, "launches": launches, "rate": clock, "clock_ghz": clock,
        "checksum": gemm_checksum(m, m, k, passes, int(flag(argv, "--seed")))})


def test_run_pair_and_report_accept_a_gemm_tenant():
    spawn = Spawner(child)
    run = run_pair(0, [{"mask": TENANTS[0]["mask"], "kind": "gemm", "passes": 2}],
                   bytes=294912, iters=3, seed=SEED, spawn=spawn)
    assert run["ok"] and run["tenants"][0]["m"] == 384
    assert flag(spawn.log[0].argv, "--kind") == "gemm"
    assert "--form" not in spawn.log[0].argv and "--operands" not in spawn.log[0].argv
    report = isolation_report(0, TENANTS, pairs=[("gemm", "gemm")], seed=SEED,
                              windows={"gemm": {"bytes": 294912, "iters": 3}},
                              spawn=Spawner(child))
    assert report["ok"], report  # the checksums were held against gemm_checksum
    for i, t in enumerate(report["pairs"]["gemm/gemm"]["tenants"]):
        assert report["solo"][i]["gemm"]["clock_ghz"] == t["solo_clock_ghz"] == 2.0
        assert t["contended_clock_ghz"] == 1.5 and t["clock_ratio"] == 0.75
        assert t["cycle_ratio"] == pytest.approx(1.0) and "form" not in t
    bad = isolation_report(0, TENANTS, pairs=[("gemm", "gemm")], seed=SEED + 1, spawn=Spawner(
        lambda n, argv, env: child(n, argv[:-1] + [str(SEED)], env)))
    assert not bad["ok"] and bad["reason"] == "bad-checksum"


def test_an_unknown_kind_and_misplaced_options_are_refused_before_spawning():
    def spawn(argv, env):
        pytest.fail(f"spawned {argv}")

    low = TENANTS[0]["mask"]
    with pytest.raises(ValueError, match="unknown tenant kind 'gem'"):
        run_pair(0, [{"mask": low, "kind": "gem"}], spawn=spawn)
    with pytest.raises(ValueError, match="not a pair of tenant kinds"):
        isolation_report(0, TENANTS, pairs=[("gemm", "gem")], spawn=spawn)
    with pytest.raises(ValueError, match="not a window of a tenant kind"):
        isolation_report(0, TENANTS, pairs=cotenancy.GEMM_PAIRS,
                         windows={"gem": {"bytes": 1}}, spawn=spawn)
    for option in ({"form": "bf16"}, {"operands": "lds"}):
        with pytest.raises(ValueError, match="a gemm tenant takes no"):
            run_pair(0, [{"mask": low, "kind": "gemm", **option}], spawn=spawn)
        with pytest.raises(ValueError, match="a gemm tenant takes no"):
            run_pair(0, [{"mask": low, **option}], ["gemm"], spawn=spawn)


def test_the_pinned_constants_are_unchanged_and_the_new_ones_stand_beside_them():
    assert cotenancy.KINDS == ("fma", "stream", "cache", "chase")
    assert cotenancy.MATRIX_KINDS == ("mfma",)
    assert cotenancy.ALL_KINDS == cotenancy.KINDS + ("mfma",)
    assert cotenancy.MFMA_OPERANDS == ("registers", "lds")
    assert cotenancy.WINDOW_KEYS == ("iters", "bytes", "passes")
    assert cotenancy.GEMM_KINDS == ("gemm",)
    assert cotenancy.EVERY_KIND == cotenancy.ALL_KINDS + ("gemm",)
    assert cotenancy.GEMM_PAIRS == (
        ("gemm", "gemm"), ("gemm", "stream"), ("stream", "gemm"), ("gemm", "fma"))
    assert cotenancy._SOLO_KEYS["gemm"] == ("clock_ghz",)
