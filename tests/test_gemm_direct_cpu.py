"""The gemm tenant's `loads` option without a GPU, on the fake children of
test_mfma_forms_cpu and test_gemm_cotenancy_cpu."""
from __future__ import annotations

import pytest

from elastic_gpu_scheduler_amd.agent.cotenancy import _child_parser, isolation_report, run_pair
from tests.test_gemm_cotenancy_cpu import child
from tests.test_mfma_forms_cpu import TENANTS, Spawner

LOW, HIGH = (t["mask"] for t in TENANTS)
WINDOW = {"bytes": 294912, "iters": 3, "seed": 0x5EED}


@pytest.mark.parametrize("wide,own,tail", (
    (None, None, ["--seed", str(0x5EED)]),
    ("direct", None, ["--loads", "direct"]),
    (None, "direct", ["--loads", "direct"]),
    ("direct", "registers", ["--loads", "registers"])))  # a tenant's own goes first
def test_a_gemm_child_is_given_loads_last_and_only_when_named(wide, own, tail):
    spawn = Spawner(lambda n, argv, env: child(n, argv, env) if "gemm" in argv
                    else Spawner().script(n, argv, env))
    tenant = {"mask": LOW, "kind": "gemm", **({"loads": own} if own else {})}
    run = run_pair(0, [tenant, {"mask": HIGH, "kind": "fma"}], loads=wide, spawn=spawn, **WINDOW)
    assert run["ok"] and spawn.log[0].argv[-2:] == tail, run
    assert "--loads" not in spawn.log[1].argv  # the call-wide value is the gemm kind's
    assert _child_parser().parse_args(spawn.log[0].argv[3:]).loads == (own or wide)


@pytest.mark.parametrize("tenant,kinds,call,message", (
    ({"kind": "stream", "loads": "direct"}, None, {}, "a stream tenant takes no loads"),
    ({"kind": "mfma", "loads": "registers"}, None, {}, "a mfma tenant takes no loads"),
    ({"loads": "direct"}, ["gemm-mxfp8"], {}, "a gemm-mxfp8 tenant takes no loads"),
    ({"kind": "gemm", "loads": "lds"}, None, {}, "unknown gemm loads 'lds'"),
    ({"kind": "fma"}, None, {"loads": "dma"}, "unknown gemm loads 'dma'")))
def test_misplaced_and_unknown_loads_are_refused_before_spawning(tenant, kinds, call, message):
    with pytest.raises(ValueError, match=message):
        run_pair(0, [{"mask": LOW, **tenant}], kinds, spawn=pytest.fail, **call)
    if call:
        with pytest.raises(ValueError, match=message):
            isolation_report(0, TENANTS, pairs=[("gemm", "fma")], spawn=pytest.fail, **call)


@pytest.mark.parametrize("wide,own,want", (
    (None, (None, None), (None, None)),
    ("direct", (None, None), ("direct", "direct")),
    (None, (None, "direct"), (None, "direct")),
    ("direct", ("registers", None), ("registers", "direct"))))
def test_gemm_entries_carry_loads_only_when_named(wide, own, want):
    tenants = [{"mask": t["mask"], **({"loads": o} if o else {})} for t, o in zip(TENANTS, own)]
    spawn = Spawner(child)
    report = isolation_report(0, tenants, pairs=[("gemm", "gemm")], loads=wide, spawn=spawn,
                              **WINDOW)
    assert report["ok"], report  # the checksum is gemm_checksum's whatever the loads
    told = [c.argv[-1] if "--loads" in c.argv else None for c in spawn.log]
    assert told == [want[0], want[1], want[0], want[1]]  # solo, solo, then the pair
    for i, t in enumerate(report["pairs"]["gemm/gemm"]["tenants"]):
        for entry in (t, report["solo"][i]["gemm"]):
            assert entry.get("loads") == want[i] and ("loads" in entry) == bool(want[i])


@pytest.mark.parametrize("argv,needs", (
    (["--co-tenancy", "--co-tenancy-gemm-loads", "direct"], "needs --co-tenancy-gemm"),
    (["--co-tenancy", "--co-tenancy-gemm", "--co-tenancy-gemm-form", "mxfp8",
      "--co-tenancy-gemm-loads", "direct"], "--co-tenancy-gemm-form are separate runs")))
def test_the_agent_flag_is_refused_where_it_measures_nothing(argv, needs, capsys):
    from elastic_gpu_scheduler_amd.cmd import agent_main

    assert agent_main.main(argv) == 2
    out, err = capsys.readouterr()
    assert out == "" and needs in err
