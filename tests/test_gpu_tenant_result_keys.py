"""The keys of cu_tenant_run's result, and their order, on a real MI355X.

A tenant's child prints the result as JSON, so the order of the keys is
output; the CPU tests run over fake children and cannot see it. One launch
per kind at the smallest window, which also pins what the probe clamps that
window to."""
from __future__ import annotations

import pytest

pytestmark = pytest.mark.gpu

HEAD = ["kind", "applied_mask", "tick_hz", "workgroups"]
TAIL = ["work_per_launch", "launches", "rate"]
LAUNCH = ["t0", "t1", "seconds", "event_seconds", "rate"]
MFMA_LAUNCH = LAUNCH + ["cycles", "ticks", "clock_ghz"]
LDS = ["operands", "lds_bytes", "lds_bytes_per_launch"]

# (case, arguments, the kind's own keys, the trailing key, a launch entry's
# keys, the clamped values)
CASES = (
    ("fma", {"kind": "fma", "iters": 1},
     ["iters"], [], LAUNCH, {"iters": 1}),
    ("stream", {"kind": "stream", "bytes": 16, "passes": 1},
     ["bytes", "passes", "checksum"], [], LAUNCH, {"bytes": 16, "passes": 1}),
    ("cache", {"kind": "cache", "bytes": 16, "passes": 1},
     ["bytes", "passes", "checksum", "bytes_per_cu"], [], LAUNCH,
     {"bytes": 16, "passes": 1}),
    ("chase", {"kind": "chase", "bytes": 128, "iters": 1},
     ["bytes", "nodes", "stride", "iters", "checksum"], ["ns_per_hop"], LAUNCH,
     {"bytes": 128, "nodes": 1, "stride": 0, "iters": 1}),
    ("mfma", {"kind": "mfma", "iters": 1},
     ["form", "iters", "checksum"], ["clock_ghz"], MFMA_LAUNCH,
     {"form": "bf16", "iters": 1}),
    ("mfma-mxfp4-lds", {"kind": "mfma", "iters": 1, "form": "mxfp4", "operands": "lds"},
     ["form", "iters", "checksum"] + LDS, ["clock_ghz"], MFMA_LAUNCH,
     {"form": "mxfp4", "iters": 1, "operands": "lds"}),
)


@pytest.fixture(scope="module")
def probe():
    from elastic_gpu_scheduler_amd._native import gpuprobe

    p = gpuprobe()  # raises loudly if the HIP extension is missing
    if p.device_count() == 0:
        pytest.fail("gpu-marked test ran but no HIP device is visible")
    return p


@pytest.mark.parametrize("case,args,own,trailing,launch,clamped", CASES,
                         ids=[c[0] for c in CASES])
def test_result_keys_and_their_order(probe, case, args, own, trailing, launch, clamped):
    r = probe.cu_tenant_run(0, launches=1, seed=1, **args)
    print(case, ":", r)
    assert list(r) == HEAD + own + TAIL + trailing
    assert r["kind"] == args["kind"]
    assert len(r["launches"]) == 1
    for entry in r["launches"]:
        assert list(entry) == launch
    for key, value in clamped.items():
        assert r[key] == value, key
