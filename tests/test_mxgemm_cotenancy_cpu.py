"""The block-scaled gemm tenants (gemm-mxfp8, gemm-mxfp4) without a GPU: the
oracle of either form against a brute-force integer product, the shape rule,
and what run_pair and isolation_report accept and refuse. The fake children
are test_mfma_forms_cpu's."""
from __future__ import annotations

import numpy as np
import pytest

from elastic_gpu_scheduler_amd.agent import cotenancy
from elastic_gpu_scheduler_amd.agent.cotenancy import (gemm_checksum, gemm_shape,
                                                       isolation_report, run_pair)
from tests.test_mfma_forms_cpu import TENANTS, FakeChild, Spawner, flag

SEED = 0x5EED
FORMS = ("mxfp8", "mxfp4")
BOUND = {"mxfp8": (14, 14), "mxfp4": (24, 12)}  # |A|, |B|, scales applied


@pytest.mark.parametrize("m,n,k,passes", ((128, 128, 128, 1), (384, 256, 640, 3),
                                          (256, 384, 96, 2)))
@pytest.mark.parametrize("form", FORMS)
def test_gemm_checksum_of_a_form_equals_the_brute_force_product(form, m, n, k, passes):
    key, fid = cotenancy._mix32(SEED ^ 0x47454D4D), cotenancy.MFMA_FORMS.index(form)
    pa = np.array([[cotenancy._mfma_a(key, i, kk, fid) for kk in range(96)]
                   for i in range(192)], dtype=np.int64)
    pb = np.array([[cotenancy._mfma_b(key, kk, j, fid) for kk in range(96)]
                   for j in range(192)], dtype=np.int64)
    assert np.abs(pa).max() <= BOUND[form][0] and np.abs(pb).max() <= BOUND[form][1]
    a = pa[np.arange(m) % 192][:, np.arange(k) % 96]
    b = pb[np.arange(n) % 192][:, np.arange(k) % 96]
    c = a @ b.T
    assert np.abs(c).max() < 1 << 23  # exact in f32
    one = int((c * np.outer(np.arange(1, m + 1), np.arange(1, n + 1))).sum())
    want = sum((1 + p) * one for p in range(passes)) % (1 << 64)
    assert gemm_checksum(m, n, k, passes, SEED, form=form) == want
    assert gemm_checksum(m, n, k, passes, SEED + 1, form=form) != want
    assert gemm_checksum(m, n, k, passes, SEED) != want


def test_bf16_is_the_default_form_and_is_unchanged():
    assert gemm_checksum(256, 256, 128, 3, SEED) == gemm_checksum(
        256, 256, 128, 3, SEED, form="bf16") == 18446744072350297156
    assert gemm_shape(294912, 3) == gemm_shape(294912, 3, form="bf16") == (384, 384, 192)
    assert gemm_shape() == gemm_shape(form="bf16") == (8192, 8192, 4096)
    for call in (gemm_shape, lambda form: gemm_checksum(128, 128, 64, 1, SEED, form=form)):
        with pytest.raises(ValueError, match="unknown gemm form 'fp8'"):
            call(form="fp8")


@pytest.mark.parametrize("form,nbytes,iters,side,k", (
    ("mxfp8", 0, 0, 8192, 4096), ("mxfp4", 0, 0, 8192, 4096),
    ("mxfp8", 0, 3, 8192, 384), ("mxfp4", 0, 3, 8192, 768),
    ("mxfp8", 1, 10**6, 128, 32768), ("mxfp4", 1, 10**6, 128, 16384),
    ("mxfp8", 1 << 40, 1, 32768, 128), ("mxfp4", 1 << 40, 1, 32768, 256),
    ("mxfp8", 256 * 500 * 3, 3, 384, 384), ("mxfp4", 256 * 500 * 3, 3, 384, 768)))
def test_gemm_shape_states_the_clamps_of_a_form(form, nbytes, iters, side, k):
    assert gemm_shape(nbytes, iters, form=form) == (side, side, k)


def child(n, argv, env):
    """An mxgemm child as the probe reports it, its clock 2.0 alone and 1.5
    from the third child on, which are the pair's."""
    kind = flag(argv, "--kind")
    form = kind[len("gemm-"):]
    m, _, k = gemm_shape(int(flag(argv, "--bytes")), int(flag(argv, "--iters")), form=form)
    passes, clock = int(flag(argv, "--passes")) or 32, 2.0 if n < 2 else 1.5
    launches = [{"t0": 1000 * i, "t1": 1000 * i + 999, "seconds": 999e-8, "rate": clock,
                 "clock_ghz": clock} for i in range(int(flag(argv, "--launches")))]
    return FakeChild(argv, env, {
        "kind": kind, "form": form, "workgroups": (m // 128) ** 2 * passes, "m": m, "n": m,
        "k": k, "passes": passes, "launches": launches, "rate": clock, "clock_ghz": clock,
        "checksum": gemm_checksum(m, m, k, passes, int(flag(argv, "--seed")), form=form)})


@pytest.mark.parametrize("kind", cotenancy.MXGEMM_KINDS)
def test_run_pair_and_report_accept_an_mxgemm_tenant(kind):
    spawn = Spawner(child)
    run = run_pair(0, [{"mask": TENANTS[0]["mask"], "kind": kind, "passes": 2}],
                   bytes=256 * 384 * 3, iters=3, seed=SEED, spawn=spawn)
    assert run["ok"] and run["tenants"][0]["m"] == 384
    assert flag(spawn.log[0].argv, "--kind") == kind
    assert "--form" not in spawn.log[0].argv and "--operands" not in spawn.log[0].argv
    pairs = cotenancy.mxgemm_pairs(kind)
    assert pairs[0] == (kind, kind) and pairs[1:] == (
        (kind, "stream"), ("stream", kind), (kind, "fma"))
    report = isolation_report(0, TENANTS, pairs=pairs[:1], seed=SEED,
                              windows={kind: {"bytes": 256 * 384 * 3, "iters": 3}},
                              spawn=Spawner(child))
    assert report["ok"], report  # the checksums were held against gemm_checksum(form=)
    for i, t in enumerate(report["pairs"][kind + "/" + kind]["tenants"]):
        assert report["solo"][i][kind]["clock_ghz"] == t["solo_clock_ghz"] == 2.0
        assert t["contended_clock_ghz"] == 1.5 and t["clock_ratio"] == 0.75
        assert t["cycle_ratio"] == pytest.approx(1.0) and "form" not in t
    bad = isolation_report(0, TENANTS, pairs=pairs[:1], seed=SEED + 1, spawn=Spawner(
        lambda n, argv, env: child(n, argv[:-1] + [str(SEED)], env)))
    assert not bad["ok"] and bad["reason"] == "bad-checksum"


@pytest.mark.parametrize("kind", cotenancy.MXGEMM_KINDS)
def test_misplaced_options_are_refused_before_spawning(kind):
    def spawn(argv, env):
        pytest.fail(f"spawned {argv}")

    low = TENANTS[0]["mask"]
    for option in ({"form": "mxfp4"}, {"operands": "lds"}):
        with pytest.raises(ValueError, match=f"a {kind} tenant takes no"):
            run_pair(0, [{"mask": low, "kind": kind, **option}], spawn=spawn)
        with pytest.raises(ValueError, match=f"a {kind} tenant takes no"):
            run_pair(0, [{"mask": low, **option}], [kind], spawn=spawn)
    with pytest.raises(ValueError, match="not a block-scaled gemm kind"):
        cotenancy.mxgemm_pairs("gemm")


def test_the_new_kinds_stand_beside_the_pinned_ones():
    assert cotenancy.MXGEMM_KINDS == ("gemm-mxfp8", "gemm-mxfp4")
    assert cotenancy.TENANT_KINDS == cotenancy.EVERY_KIND + cotenancy.MXGEMM_KINDS
    assert all(cotenancy._SOLO_KEYS[kind] == ("clock_ghz",) for kind in cotenancy.MXGEMM_KINDS)
    assert cotenancy._child_parser().parse_args(
        ["--child", "--kind", "gemm-mxfp4"]).kind == "gemm-mxfp4"
