"""The decode tenants (decode-mxfp8, decode-mxfp4) without a GPU: the oracle at
32 rows against a brute-force integer product, the shape rule, and what
run_pair, isolation_report and the agent accept and refuse. The fake
children are test_mfma_forms_cpu's."""
from __future__ import annotations

import numpy as np
import pytest

from elastic_gpu_scheduler_amd.agent import cotenancy
from elastic_gpu_scheduler_amd.agent.cotenancy import (decode_pairs, decode_shape,
                                                       gemm_checksum, isolation_report, run_pair)
from tests.test_mfma_forms_cpu import TENANTS, FakeChild, Spawner, flag

SEED = 0x5EED


@pytest.mark.parametrize("form,n,k,passes", (("mxfp8", 384, 640, 3), ("mxfp4", 256, 768, 2)))
def test_gemm_checksum_at_32_rows_equals_the_brute_force_product(form, n, k, passes):
    key, fid = cotenancy._mix32(SEED ^ 0x47454D4D), cotenancy.MFMA_FORMS.index(form)
    a = np.array([[cotenancy._mfma_a(key, i, kk % 96, fid) for kk in range(k)]
                  for i in range(32)], dtype=np.int64)
    w = np.array([[cotenancy._mfma_b(key, kk % 96, j % 192, fid) for kk in range(k)]
                  for j in range(n)], dtype=np.int64)
    c = a @ w.T
    assert np.abs(c).max() < 1 << 23  # exact in f32
    one = int((c * np.outer(np.arange(1, 33), np.arange(1, n + 1))).sum())
    want = one * (passes * (passes + 1) // 2) % (1 << 64)
    assert gemm_checksum(32, n, k, passes, SEED, form=form) == want


@pytest.mark.parametrize("form,nbytes,iters,n,k", (
    ("mxfp8", 0, 0, 131072, 8192), ("mxfp4", 0, 0, 262144, 8192),
    ("mxfp8", 1, 10**6, 128, 32768), ("mxfp4", 1, 10**6, 128, 16384),
    ("mxfp8", 1 << 40, 1, 1 << 20, 128), ("mxfp4", 1 << 40, 1, 1 << 20, 256),
    ("mxfp8", 128 * 500 * 3, 3, 384, 384), ("mxfp4", 128 * 500 * 3, 3, 384, 768)))
def test_decode_shape_states_the_clamps(form, nbytes, iters, n, k):
    assert decode_shape(nbytes, iters, form) == (32, n, k)


def test_decode_shape_refuses_a_form_without_scales():
    with pytest.raises(ValueError, match="block-scaled"):
        decode_shape(form="bf16")


def child(n, argv, env):
    """A decode child as the probe reports it, its clock 2.0 alone and 1.5
    from the third child on, which are the pair's."""
    kind = flag(argv, "--kind")
    form = kind[len("decode-"):]
    m, cols, k = decode_shape(int(flag(argv, "--bytes")), int(flag(argv, "--iters")), form)
    passes, clock = int(flag(argv, "--passes")) or 48, 2.0 if n < 2 else 1.5
    launches = [{"t0": 1000 * i, "t1": 1000 * i + 999, "seconds": 999e-8, "rate": clock,
                 "clock_ghz": clock} for i in range(int(flag(argv, "--launches")))]
    return FakeChild(argv, env, {
        "kind": kind, "form": form, "workgroups": cols // 128 * passes, "m": m, "n": cols,
        "k": k, "passes": passes, "launches": launches, "rate": clock, "clock_ghz": clock,
        "checksum": gemm_checksum(m, cols, k, passes, int(flag(argv, "--seed")), form=form)})


@pytest.mark.parametrize("kind", cotenancy.DECODE_KINDS)
def test_run_pair_and_report_accept_a_decode_tenant(kind):
    window = {"bytes": 128 * 384 * 3, "iters": 3}
    spawn = Spawner(child)
    run = run_pair(0, [{"mask": TENANTS[0]["mask"], "kind": kind, "passes": 2}], seed=SEED,
                   spawn=spawn, **window)
    assert run["ok"] and (run["tenants"][0]["m"], run["tenants"][0]["n"]) == (32, 384)
    assert spawn.log[0].argv[-14:] == [
        "--device", "0", "--kind", kind, "--launches", "8", "--iters", "3", "--bytes",
        str(window["bytes"]), "--passes", "2", "--seed", str(SEED)]
    pairs = decode_pairs(kind)
    assert pairs == ((kind, kind), (kind, "stream"), ("stream", kind), (kind, "gemm"),
                     ("gemm", kind))
    report = isolation_report(0, TENANTS, pairs=pairs[:1], seed=SEED, windows={kind: window},
                              spawn=Spawner(child))
    assert report["ok"], report  # the checksums were held against gemm_checksum(32, ...)
    for i, t in enumerate(report["pairs"][kind + "/" + kind]["tenants"]):
        assert report["solo"][i][kind]["clock_ghz"] == t["solo_clock_ghz"] == 2.0
        assert t["contended_clock_ghz"] == 1.5 and t["clock_ratio"] == 0.75
        assert t["cycle_ratio"] == pytest.approx(1.0)
    bad = isolation_report(0, TENANTS, pairs=pairs[:1], seed=SEED + 1, spawn=Spawner(
        lambda n, argv, env: child(n, argv[:-1] + [str(SEED)], env)))
    assert not bad["ok"] and bad["reason"] == "bad-checksum"


@pytest.mark.parametrize("kind", cotenancy.DECODE_KINDS)
@pytest.mark.parametrize("option", ({"form": "mxfp4"}, {"operands": "lds"}, {"loads": "direct"}))
def test_misplaced_options_are_refused_before_spawning(kind, option):
    def spawn(argv, env):
        pytest.fail(f"spawned {argv}")

    low = TENANTS[0]["mask"]
    with pytest.raises(ValueError, match=f"a {kind} tenant takes no"):
        run_pair(0, [{"mask": low, "kind": kind, **option}], spawn=spawn)
    with pytest.raises(ValueError, match=f"a {kind} tenant takes no"):
        run_pair(0, [{"mask": low, **option}], [kind], spawn=spawn)


@pytest.mark.parametrize("argv,needs", (
    (["--co-tenancy-decode"], "--co-tenancy-decode needs --co-tenancy"),
    (["--co-tenancy", "--co-tenancy-decode", "mxfp8", "--co-tenancy-gemm"],
     "--co-tenancy-decode and --co-tenancy-gemm are separate runs"),
    (["--co-tenancy", "--co-tenancy-decode", "--co-tenancy-mfma"],
     "--co-tenancy-decode and --co-tenancy-mfma are separate runs")))
def test_the_agent_flag_is_refused_where_it_measures_nothing(argv, needs, capsys):
    from elastic_gpu_scheduler_amd.cmd import agent_main

    assert agent_main.main(argv) == 2
    out, err = capsys.readouterr()
    assert out == "" and needs in err
    assert agent_main.build_parser().parse_args(
        ["--co-tenancy", "--co-tenancy-decode"]).co_tenancy_decode == ("mxfp4",)


def test_the_new_kinds_stand_beside_the_pinned_ones():
    assert cotenancy.DECODE_KINDS == ("decode-mxfp8", "decode-mxfp4")
    assert cotenancy.CO_KINDS == cotenancy.TENANT_KINDS + cotenancy.DECODE_KINDS
    assert all(cotenancy._SOLO_KEYS[kind] == ("clock_ghz",) for kind in cotenancy.DECODE_KINDS)
    assert cotenancy._child_parser().parse_args(
        ["--child", "--kind", "decode-mxfp4"]).kind == "decode-mxfp4"
    with pytest.raises(ValueError, match="not a decode kind"):
        decode_pairs("gemm-mxfp4")
