"""The decode tenants' `weights` option without a GPU, on the fake children of
test_mfma_forms_cpu and test_decode_cotenancy_cpu."""
from __future__ import annotations

import pytest

from elastic_gpu_scheduler_amd.agent.cotenancy import DECODE_KINDS, isolation_report, run_pair
from tests.test_decode_cotenancy_cpu import child
from tests.test_mfma_forms_cpu import TENANTS, Spawner

LOW, HIGH = (t["mask"] for t in TENANTS)
WINDOW = {"bytes": 128 * 384 * 3, "iters": 3, "seed": 0x5EED}


@pytest.mark.parametrize("kind", DECODE_KINDS)
@pytest.mark.parametrize("wide,own,tail", (
    (None, None, ["--seed", str(0x5EED)]),
    ("tiled", None, ["--weights", "tiled"]),
    (None, "tiled", ["--weights", "tiled"]),
    ("tiled", "rows", ["--weights", "rows"])))  # a tenant's own goes first
def test_a_decode_child_is_given_weights_last_and_only_when_named(kind, wide, own, tail):
    spawn = Spawner(lambda n, argv, env: child(n, argv, env) if kind in argv
                    else Spawner().script(n, argv, env))
    tenant = {"mask": LOW, "kind": kind, **({"weights": own} if own else {})}
    run = run_pair(0, [tenant, {"mask": HIGH, "kind": "fma"}], weights=wide, spawn=spawn,
                   **WINDOW)
    assert run["ok"] and spawn.log[0].argv[-2:] == tail, run
    assert "--weights" not in spawn.log[1].argv  # the call-wide value is the decode kinds'


@pytest.mark.parametrize("tenant,kinds,call,message", (
    ({"kind": "stream", "weights": "tiled"}, None, {}, "a stream tenant takes no weights"),
    ({"weights": "tiled"}, ["gemm-mxfp4"], {}, "a gemm-mxfp4 tenant takes no weights"),
    ({"kind": "decode-mxfp4", "weights": "direct"}, None, {}, "unknown decode weights 'direct'"),
    ({"kind": "fma"}, None, {"weights": "columns"}, "unknown decode weights 'columns'")))
def test_misplaced_and_unknown_weights_are_refused_before_spawning(tenant, kinds, call, message):
    with pytest.raises(ValueError, match=message):
        run_pair(0, [{"mask": LOW, **tenant}], kinds, spawn=pytest.fail, **call)
    if "unknown" in message:  # a report's tenants have no kind of their own to misplace it on
        own = {k: v for k, v in tenant.items() if k != "kind"}
        with pytest.raises(ValueError, match=message):
            isolation_report(0, [{"mask": LOW, **own}, TENANTS[1]],
                             pairs=[("decode-mxfp4", "fma")], spawn=pytest.fail, **call)


def test_the_agent_flag_is_refused_without_the_decode_run(capsys):
    from elastic_gpu_scheduler_amd.cmd import agent_main

    assert agent_main.main(["--co-tenancy", "--co-tenancy-decode-weights", "tiled"]) == 2
    out, err = capsys.readouterr()
    assert out == "" and "--co-tenancy-decode-weights needs --co-tenancy-decode" in err
