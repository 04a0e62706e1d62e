"""The attention-decode tenant without a GPU: the shape, split and length
rules, the new tuples and pairs beside the pinned ones, and what run_pair,
isolation_report and the agent accept and refuse. The fake children are
test_mfma_forms_cpu's."""
from __future__ import annotations

import pytest

from elastic_gpu_scheduler_amd.agent import cotenancy
from elastic_gpu_scheduler_amd.agent.cotenancy import (ATTENTION_TOLERANCE,
                                                       attention_decode_length,
                                                       attention_decode_pairs,
                                                       attention_decode_shape, isolation_report,
                                                       run_pair)
from tests.test_mfma_forms_cpu import TENANTS, FakeChild, Spawner, flag

SEED = 0x5EED
KIND = "attention-decode"


def window_bytes(iters, heads):
    return heads * (512 * 128 * iters + 4096)


@pytest.mark.parametrize("nbytes,iters,shape", (
    (0, 0, (256, 8192, 128, 8)), (1, 10**6, (1, 32768, 128, 32)),
    (1 << 50, 1, (1024, 128, 128, 1)), (window_bytes(9, 2) + 4095, 9, (2, 1152, 128, 2)),
    (window_bytes(17, 3), 17, (3, 2176, 128, 3)),
    (window_bytes(3, 700), 3, (700, 384, 128, 1)),    # 2048 // 700 = 2, but ceil(3 / 8) = 1
    (window_bytes(17, 700), 17, (700, 2176, 128, 2)),  # uneven: spans of 9 and 8 units
    (window_bytes(64, 512), 64, (512, 8192, 128, 4))))
def test_the_shape_rule_states_the_defaults_the_clamps_and_the_splits(nbytes, iters, shape):
    assert attention_decode_shape(nbytes, iters) == shape


def test_lengths_are_ragged_and_cover_every_residue():
    assert [attention_decode_length(h, 128) for h in (0, 1, 2, 3, 83)] == [128, 91, 54, 17, 1]
    assert attention_decode_length(1, 8192) == 8192 - 37
    assert sorted(attention_decode_length(h, 128) for h in range(128)) == list(range(1, 129))


def test_the_new_kind_stands_beside_the_pinned_ones():
    assert cotenancy.ATTENTION_DECODE_KINDS == (KIND,)
    assert cotenancy.SERVING_KINDS == cotenancy.WORKLOAD_KINDS + (KIND,)
    assert cotenancy.ATTENTION_KINDS == ("attention",)
    assert cotenancy.WORKLOAD_KINDS == cotenancy.CO_KINDS + ("attention",)
    assert cotenancy._SOLO_KEYS[KIND] == ("clock_ghz",)
    assert attention_decode_pairs() == (
        (KIND, KIND), (KIND, "stream"), ("stream", KIND), (KIND, "attention"),
        ("attention", KIND), (KIND, "decode-mxfp4"), ("decode-mxfp4", KIND))
    assert cotenancy._child_parser().parse_args(["--child", "--kind", KIND]).kind == KIND


def child(error):
    """A child's report: clock 2.0 alone, 1.5 from the third child on."""
    def make(n, argv, env):
        clock = 2.0 if n < 2 else 1.5
        launches = [{"t0": 1000 * i, "t1": 1000 * i + 999, "seconds": 999e-8, "rate": clock,
                     "clock_ghz": clock} for i in range(int(flag(argv, "--launches")))]
        return FakeChild(argv, env, {
            "kind": KIND, "workgroups": 6, "launches": launches, "rate": clock,
            "clock_ghz": clock, "max_error": error})
    return make


def test_run_pair_and_report_accept_an_attention_decode_tenant():
    window = {"bytes": window_bytes(9, 2), "iters": 9}
    spawn = Spawner(child(0.002))
    run = run_pair(0, [{"mask": TENANTS[0]["mask"], "kind": KIND, "passes": 2}],
                   seed=SEED, spawn=spawn, **window)
    assert run["ok"] and run["tenants"][0]["max_error"] == 0.002
    assert spawn.log[0].argv[-14:] == [  # the window and no option
        "--device", "0", "--kind", KIND, "--launches", "8", "--iters", "9", "--bytes",
        str(window["bytes"]), "--passes", "2", "--seed", str(SEED)]
    pairs, name = attention_decode_pairs()[:1], KIND + "/" + KIND
    report = isolation_report(0, TENANTS, pairs=pairs, seed=SEED, spawn=Spawner(child(0.002)),
                              windows={KIND: window})
    assert report["ok"], report
    for i, t in enumerate(report["pairs"][name]["tenants"]):
        assert report["solo"][i][KIND]["clock_ghz"] == t["solo_clock_ghz"] == 2.0
        assert t["contended_clock_ghz"] == 1.5 and t["clock_ratio"] == 0.75
        assert t["cycle_ratio"] == pytest.approx(1.0)
    for error in (2 * ATTENTION_TOLERANCE, float("nan")):
        bad = isolation_report(0, TENANTS, pairs=pairs, spawn=Spawner(child(error)))
        assert not bad["ok"] and bad["reason"] == "bad-output"
        assert bad["pairs"][name]["tenants"][0]["ratio"] == 0.75  # kept


@pytest.mark.parametrize("option", ({"form": "mxfp4"}, {"operands": "lds"},
                                    {"loads": "direct"}, {"weights": "tiled"}))
def test_misplaced_options_are_refused_before_spawning(option):
    def spawn(argv, env):
        pytest.fail(f"spawned {argv}")

    with pytest.raises(ValueError, match="a attention-decode tenant takes no"):
        run_pair(0, [{"mask": TENANTS[0]["mask"], "kind": KIND, **option}], spawn=spawn)


FLAG = "--co-tenancy-attention-decode"


@pytest.mark.parametrize("argv,needs", (
    ([FLAG], FLAG + " needs --co-tenancy"),
    *((["--co-tenancy", FLAG, *other], f"{FLAG} and {other[0]} are separate runs")
      for other in (["--co-tenancy-cache"], ["--co-tenancy-chase"], ["--co-tenancy-mfma"],
                    ["--co-tenancy-gemm"], ["--co-tenancy-decode", "mxfp8"],
                    ["--co-tenancy-attention"]))))
def test_the_agent_flag_is_refused_where_it_measures_nothing(argv, needs, capsys, monkeypatch):
    from elastic_gpu_scheduler_amd.agent.agent import NodeAgent
    from elastic_gpu_scheduler_amd.cmd import agent_main

    monkeypatch.setattr(NodeAgent, "verify_isolation",
                        lambda *a, **k: pytest.fail("started a report"))
    assert agent_main.main(argv) == 2
    out, err = capsys.readouterr()
    assert out == "" and needs in err
    assert agent_main.build_parser().parse_args(
        ["--co-tenancy", FLAG]).co_tenancy_attention_decode is True
