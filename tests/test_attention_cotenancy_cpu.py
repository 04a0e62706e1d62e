"""The attention tenant without a GPU: the shape rule, the data rule, the new
tuples and pairs, and what run_pair, isolation_report and the agent accept
and refuse. The fake children are test_mfma_forms_cpu's."""
from __future__ import annotations

import pytest

from elastic_gpu_scheduler_amd.agent import cotenancy
from elastic_gpu_scheduler_amd.agent.cotenancy import (ATTENTION_TOLERANCE, attention_operands,
                                                       attention_pairs, attention_shape,
                                                       isolation_report, run_pair)
from tests.test_mfma_forms_cpu import TENANTS, FakeChild, Spawner, flag

SEED = 0x5EED


@pytest.mark.parametrize("nbytes,iters,shape", (
    (0, 0, (64, 8192, 128)), (1, 10**6, (1, 32768, 128)), (1 << 50, 1, (1024, 128, 128)),
    (768 * 384 * 2 + 767, 3, (2, 384, 128)), (768 * 640 * 3, 5, (3, 640, 128))))
def test_attention_shape_states_the_defaults_and_the_clamps(nbytes, iters, shape):
    assert attention_shape(nbytes, iters) == shape


def test_attention_operands_are_small_multiples_that_differ():
    q, k, v = attention_operands(SEED, 0, 4)
    for rows, scale in ((q, 8), (k, 4), (v, 16)):
        assert len(rows) == 4 and all(len(row) == 128 for row in rows)
        scaled = [x * scale for row in rows for x in row]
        assert all(x == int(x) and -15 <= x <= 15 for x in scaled)
        assert len(set(scaled)) > 16
    assert [[x * 8 for x in row] for row in q] != [[x * 4 for x in row] for row in k]
    assert attention_operands(SEED + 1, 0, 4) != (q, k, v)
    assert attention_operands(SEED, 1, 4)[0] != q
    assert attention_operands(SEED, 0, 2) == (q[:2], k[:2], v[:2])
    # one element by hand: K (which = 1) of head 3 at row 2, d = 5
    key = cotenancy._mix32(cotenancy._mix32(SEED ^ 0x4154544E) ^ 0x9E3779B1 ^ 3)
    assert attention_operands(SEED, 3, 3)[1][2][5] == (
        cotenancy._mix32(key ^ (2 << 7 | 5)) % 31 - 15) / 4


def test_the_new_kind_stands_beside_the_pinned_ones():
    assert cotenancy.ATTENTION_KINDS == ("attention",)
    assert cotenancy.WORKLOAD_KINDS == cotenancy.CO_KINDS + ("attention",)
    assert "attention" not in cotenancy.CO_KINDS
    assert cotenancy._SOLO_KEYS["attention"] == ("clock_ghz",)
    assert ATTENTION_TOLERANCE == 2 ** -7
    assert attention_pairs() == (
        ("attention", "attention"), ("attention", "stream"), ("stream", "attention"),
        ("attention", "gemm"), ("gemm", "attention"), ("attention", "decode-mxfp4"),
        ("decode-mxfp4", "attention"))
    assert cotenancy._child_parser().parse_args(
        ["--child", "--kind", "attention"]).kind == "attention"


def child(error):
    """An attention child as the probe reports it, its clock 2.0 alone and 1.5
    from the third child on, which are the pair's."""
    def make(n, argv, env):
        clock = 2.0 if n < 2 else 1.5
        launches = [{"t0": 1000 * i, "t1": 1000 * i + 999, "seconds": 999e-8, "rate": clock,
                     "clock_ghz": clock} for i in range(int(flag(argv, "--launches")))]
        return FakeChild(argv, env, {
            "kind": "attention", "workgroups": 6, "launches": launches, "rate": clock,
            "clock_ghz": clock, "max_error": error})
    return make


def test_run_pair_and_report_accept_an_attention_tenant():
    window = {"bytes": 768 * 384 * 2, "iters": 3}
    spawn = Spawner(child(0.002))
    run = run_pair(0, [{"mask": TENANTS[0]["mask"], "kind": "attention", "passes": 2}],
                   seed=SEED, spawn=spawn, **window)
    assert run["ok"] and run["tenants"][0]["max_error"] == 0.002
    assert spawn.log[0].argv[-14:] == [  # the window and no option
        "--device", "0", "--kind", "attention", "--launches", "8", "--iters", "3", "--bytes",
        str(window["bytes"]), "--passes", "2", "--seed", str(SEED)]
    pairs = attention_pairs()[:1]
    report = isolation_report(0, TENANTS, pairs=pairs, seed=SEED, spawn=Spawner(child(0.002)),
                              windows={"attention": window})
    assert report["ok"], report
    for i, t in enumerate(report["pairs"]["attention/attention"]["tenants"]):
        assert report["solo"][i]["attention"]["clock_ghz"] == t["solo_clock_ghz"] == 2.0
        assert t["contended_clock_ghz"] == 1.5 and t["clock_ratio"] == 0.75
        assert t["cycle_ratio"] == pytest.approx(1.0)
    for error in (2 * ATTENTION_TOLERANCE, float("nan")):
        bad = isolation_report(0, TENANTS, pairs=pairs, spawn=Spawner(child(error)))
        assert not bad["ok"] and bad["reason"] == "bad-output"
        assert bad["pairs"]["attention/attention"]["tenants"][0]["ratio"] == 0.75  # kept


@pytest.mark.parametrize("option", ({"form": "mxfp4"}, {"operands": "lds"},
                                    {"loads": "direct"}, {"weights": "tiled"}))
def test_misplaced_options_are_refused_before_spawning(option):
    def spawn(argv, env):
        pytest.fail(f"spawned {argv}")

    with pytest.raises(ValueError, match="a attention tenant takes no"):
        run_pair(0, [{"mask": TENANTS[0]["mask"], "kind": "attention", **option}], spawn=spawn)


@pytest.mark.parametrize("argv,needs", (
    (["--co-tenancy-attention"], "--co-tenancy-attention needs --co-tenancy"),
    *((["--co-tenancy", "--co-tenancy-attention", *other],
       f"--co-tenancy-attention and {other[0]} are separate runs")
      for other in (["--co-tenancy-cache"], ["--co-tenancy-chase"], ["--co-tenancy-mfma"],
                    ["--co-tenancy-gemm"], ["--co-tenancy-decode", "mxfp8"]))))
def test_the_agent_flag_is_refused_where_it_measures_nothing(argv, needs, capsys, monkeypatch):
    from elastic_gpu_scheduler_amd.agent.agent import NodeAgent
    from elastic_gpu_scheduler_amd.cmd import agent_main

    monkeypatch.setattr(NodeAgent, "verify_isolation",
                        lambda *a, **k: pytest.fail("started a report"))
    assert agent_main.main(argv) == 2
    out, err = capsys.readouterr()
    assert out == "" and needs in err
    assert agent_main.build_parser().parse_args(
        ["--co-tenancy", "--co-tenancy-attention"]).co_tenancy_attention is True
