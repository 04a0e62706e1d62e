"""Deep card self-test, the parts that need no GPU: the pattern definition,
the health verdict, and the publish -> annotation -> scheduler status path."""
from __future__ import annotations

import json

import pytest

from elastic_gpu_scheduler_amd._native import core, gpuprobe, gpuprobe_available
from elastic_gpu_scheduler_amd.agent import inventory as inv
from elastic_gpu_scheduler_amd.agent import topology as topo
from elastic_gpu_scheduler_amd.agent.agent import NodeAgent
from elastic_gpu_scheduler_amd.agent.health import HealthLimits, evaluate_card
from elastic_gpu_scheduler_amd.k8s import objects as obj
from elastic_gpu_scheduler_amd.k8s.client import FakeKubeClient
from elastic_gpu_scheduler_amd.utils import types as t

GiB = 1024**3
M64 = (1 << 64) - 1

needs_probe = pytest.mark.skipif(not gpuprobe_available(),
                                 reason="_gpuprobe extension not built")


def splitmix(seed: int, w: int) -> int:
    """Independent definition of the pattern: splitmix64 finaliser."""
    z = (seed + (w + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


# --- pattern ---------------------------------------------------------------

@needs_probe
@pytest.mark.parametrize("seed", [0, 1, M64])
def test_pattern_word_matches_splitmix64(seed):
    p = gpuprobe()
    for w in (0, 1, 2**32, 2**61):
        assert p.pattern_word(seed, w) == splitmix(seed, w), (seed, w)


@needs_probe
@pytest.mark.parametrize("seed", [0, 1, M64])
def test_pattern_xor_matches_splitmix64(seed):
    p = gpuprobe()
    for first in (0, 1, 2**32, 2**61):
        want = 0
        for w in range(first, first + 1000):
            want ^= splitmix(seed, w)
        assert p.pattern_xor(seed, first, 1000) == want, (seed, first)
    assert p.pattern_xor(seed, 7, 0) == 0
    assert p.pattern_xor(seed, 7, 1) == splitmix(seed, 7)


@needs_probe
def test_probes_raise_without_device():
    import torch

    if torch.cuda.is_available():
        return  # a device is visible: covered by the gpu-marked tests
    p = gpuprobe()
    with pytest.raises(RuntimeError):
        p.stamp(0, 1, 16)
    with pytest.raises(RuntimeError):
        p.hbm_pattern_test(0, 1 << 20, 1)
    with pytest.raises(RuntimeError):
        p.xcd_bandwidth(0, 1, 2, 64)
    with pytest.raises(RuntimeError):
        p.mfma_selftest(0, 4)


# --- evaluate_card ---------------------------------------------------------

def clean_report(n_xcd: int = 8) -> dict:
    return {
        "index": 0,
        "hbm_gbps": 6100.0,
        "pattern": {"bytes": GiB, "mismatches": [0, 0], "records": [],
                    "seconds": 0.001, "gbps": 4000.0},
        "xcd": [{"xcc": x, "workgroups": 128, "chunks": 512,
                 "expected_chunks": 512, "bytes": 128 << 20,
                 "seconds": 2e-4, "gbps": 650.0 + x, "checksum": 0xABC0 + x,
                 "expected_checksum": 0xABC0 + x, "stable": True}
                for x in range(n_xcd)],
        "mfma": [{"xcc": x, "workgroups": 128, "mismatched_elements": 0}
                 for x in range(n_xcd)],
    }


def test_evaluate_clean_card_is_healthy():
    assert evaluate_card(clean_report(), HealthLimits()) == {
        "healthy": True, "reasons": []}
    assert evaluate_card(clean_report(1), HealthLimits())["healthy"]


def _with(mutate) -> dict:
    r = clean_report()
    mutate(r)
    return r


@pytest.mark.parametrize("mutate,reason", [
    (lambda r: r.update(hbm_gbps=240.0), "hbm-bandwidth"),
    (lambda r: r["pattern"].update(mismatches=[0, 1]), "hbm-data"),
    (lambda r: r["pattern"].update(mismatches=[3, 0]), "hbm-data"),
    (lambda r: r["mfma"][4].update(mismatched_elements=32), "mfma"),
    (lambda r: r["xcd"][5].update(gbps=300.0), "xcd-slow:5"),
    (lambda r: r["xcd"][6].update(checksum=1), "xcd-checksum:6"),
    (lambda r: r["xcd"][6].update(stable=False), "xcd-checksum:6"),
    (lambda r: r["xcd"][7].update(chunks=511), "xcd-chunks:7"),
])
def test_evaluate_single_defect_gives_exactly_its_reason(mutate, reason):
    assert evaluate_card(_with(mutate), HealthLimits()) == {
        "healthy": False, "reasons": [reason]}


def test_evaluate_xcd_ratio_boundary_and_limit():
    # 0.5 x the median is the limit itself: not below it, so healthy.
    r = clean_report()
    for e in r["xcd"]:
        e["gbps"] = 600.0
    r["xcd"][3]["gbps"] = 300.0
    assert evaluate_card(r, HealthLimits())["healthy"]
    r["xcd"][3]["gbps"] = 299.0
    assert evaluate_card(r, HealthLimits())["reasons"] == ["xcd-slow:3"]
    assert evaluate_card(r, HealthLimits(xcd_ratio=0.25))["healthy"]


def test_evaluate_xcd_ratio_inert_below_three_xcds():
    r = clean_report(2)
    r["xcd"][1]["gbps"] = 1.0
    assert evaluate_card(r, HealthLimits())["healthy"]
    # ... while checksum and chunk checks still apply to a lone XCD.
    r = clean_report(1)
    r["xcd"][0]["checksum"] ^= 1
    assert evaluate_card(r, HealthLimits())["reasons"] == ["xcd-checksum:0"]


def test_evaluate_skipped_subreport_is_not_a_reason():
    r = clean_report()
    r["pattern"] = {"skipped": "insufficient free memory", "bytes": GiB,
                    "free_bytes": 123}
    assert evaluate_card(r, HealthLimits()) == {"healthy": True, "reasons": []}
    r["xcd"] = {"skipped": "insufficient free memory"}
    r["mfma"] = None
    assert evaluate_card(r, HealthLimits())["healthy"]


def test_evaluate_hbm_threshold_is_the_agents():
    from elastic_gpu_scheduler_amd.agent import agent as agent_mod

    assert HealthLimits().hbm_gbps == agent_mod.HBM_HEALTH_THRESHOLD_GBPS == 1000.0
    assert HealthLimits().xcd_ratio == 0.5


# --- NodeAgent.self_test over a fake probe ----------------------------------

class FakeProbe:
    """Stands in for the HIP module: two healthy cards, the second too full
    for the memory-hungry sub-tests."""
    XCD_PATTERN_SEED = 99

    def __init__(self):
        self.calls = []

    def device_count(self):
        return 2

    def hbm_bandwidth(self, device, mib, iters):
        return 6000.0

    def hbm_pattern_test(self, device, nbytes, seed):
        self.calls.append(("pattern", device, nbytes))
        if device == 1:
            return {"skipped": "insufficient free memory", "bytes": nbytes,
                    "free_bytes": 5}
        return {"bytes": nbytes, "mismatches": [0, 0], "records": [],
                "seconds": 1e-3, "gbps": 4000.0}

    @staticmethod
    def _xor(seed, first, n):
        return (seed * 1000003 + first * 31 + n) & M64

    def pattern_xor(self, seed, first, n):
        return self._xor(seed, first, n)

    def xcd_bandwidth(self, device, slice_mib, iters, chunk_kib):
        self.calls.append(("xcd", device, slice_mib, iters, chunk_kib))
        if device == 1:
            raise RuntimeError("xcd_bandwidth: insufficient free device memory")
        words = slice_mib * 2**20 // 8
        return [{"xcc": x, "workgroups": 128, "chunks": slice_mib * 4,
                 "bytes": slice_mib << 20, "seconds": 1e-4, "gbps": 700.0,
                 "checksum": self._xor(99, x * words, words),
                 "stable": True} for x in range(8)]

    def mfma_selftest(self, device, iters):
        self.calls.append(("mfma", device, iters))
        return [{"xcc": x, "workgroups": 128, "mismatched_elements": 0}
                for x in range(8)]


def test_self_test_builds_reports_and_tolerates_full_card(monkeypatch):
    import elastic_gpu_scheduler_amd._native as native
    from elastic_gpu_scheduler_amd.agent.agent import health_summary

    fake = FakeProbe()
    monkeypatch.setattr(native, "_gpuprobe", fake)
    monkeypatch.setattr(native, "_gpuprobe_tried", True)
    report = NodeAgent("n").self_test()
    assert ("pattern", 0, 1024 * 2**20) in fake.calls      # defaults: 1 GiB,
    assert ("xcd", 0, 128, 3, 256) in fake.calls           # 128 MiB slices,
    assert ("mfma", 0, 256) in fake.calls                  # 256 iterations
    assert [r["index"] for r in report] == [0, 1]
    assert all(r["healthy"] and r["reasons"] == [] for r in report)
    assert all(e["expected_chunks"] == 512 and
               e["expected_checksum"] == e["checksum"] for e in report[0]["xcd"])
    assert "skipped" in report[1]["pattern"] and "skipped" in report[1]["xcd"]
    s = health_summary(report[1])
    assert s["xcd_gbps"] == {} and s["hbm_mismatches"] is None and s["healthy"]

    # A wrong checksum from the card is caught against the host's pattern.
    bad = FakeProbe()
    bad.pattern_xor = lambda seed, first, n: 1
    monkeypatch.setattr(native, "_gpuprobe", bad)
    broken = NodeAgent("n").self_test(slice_mib=8)[0]
    assert broken["reasons"] == [f"xcd-checksum:{x}" for x in range(8)]
    # Any other probe failure is not swallowed.
    bad.xcd_bandwidth = lambda *a: (_ for _ in ()).throw(RuntimeError("HIP error"))
    with pytest.raises(RuntimeError):
        NodeAgent("n").self_test()


# --- publish -> annotation -> scheduler ------------------------------------

@pytest.fixture
def four_card_agent(monkeypatch):
    cards = [{"index": i, "memory_bytes": 288 * GiB, "core": 100}
             for i in range(4)]
    monkeypatch.setattr(inv, "discover", lambda prefer="auto": cards)
    monkeypatch.setattr(topo, "discover",
                        lambda n, prefer="auto": topo.default_hive(n))
    client = FakeKubeClient()
    client.add_node({"metadata": {"name": "gpu-node"}, "status": {}})
    return client, NodeAgent("gpu-node", client)


def _fake_self_test(self, pattern_mib=1024, slice_mib=128, mfma_iters=256):
    out = []
    for i in range(4):
        r = clean_report()
        r["index"] = i
        if i == 2:
            r["pattern"]["mismatches"] = [0, 5]
            r["pattern"]["records"] = [(1, 77, 1 << 40)]
        r.update(evaluate_card(r, HealthLimits()))
        out.append(r)
    return out


def test_publish_deep_marks_sick_card_and_explains_it(four_card_agent,
                                                      monkeypatch):
    from elastic_gpu_scheduler_amd.scheduler.service import SchedulerRegistry
    from tests.conftest import make_pod

    client, agent = four_card_agent
    monkeypatch.setattr(NodeAgent, "self_test", _fake_self_test)
    monkeypatch.setattr(NodeAgent, "health_check", lambda *a, **k: pytest.fail(
        "deep mode must not fall back to the bandwidth-only check"))
    out = agent.publish_with_health(deep=True)
    assert out["sick"] == [2]

    node = client.get_node("gpu-node")
    devs = obj.node_devices(node)
    assert len(devs) == 4
    assert [d.schedulable() for d in devs] == [True, True, False, True]
    assert node["status"]["allocatable"]["elasticgpu.io/gpu-core"] == "300"
    assert node["status"]["allocatable"]["amd.com/gpu"] == "3"

    # The annotation: compact, every card, no raw records.
    raw = node["metadata"]["annotations"][t.ANNOTATION_NODE_HEALTH]
    assert t.ANNOTATION_NODE_HEALTH == "elasticgpu.io/gpu-health"
    assert ", " not in raw and "records" not in raw
    cards = json.loads(raw)["cards"]
    assert [c["index"] for c in cards] == [0, 1, 2, 3]
    assert cards[2]["reasons"] == ["hbm-data"] and not cards[2]["healthy"]
    assert cards[2]["hbm_mismatches"] == [0, 5]
    assert cards[0]["xcd_gbps"]["7"] == 657.0 and cards[0]["ts"] > 0
    assert obj.node_card_health(node) == {2: ["hbm-data"]}

    registry = SchedulerRegistry(client)
    sch = registry.default
    pod = client.create_pod(make_pod("three", core=300))
    ok, failed = sch.assume(["gpu-node"], pod)
    assert ok == ["gpu-node"], failed
    sch.bind("gpu-node", pod)
    allocation = obj.parse_allocation(client.get_pod("default", "three"))
    assert sorted(allocation[0]) == [0, 1, 3]
    status = sch.status()["nodes"]["gpu-node"]
    assert status["unhealthy_cards"] == {2: ["hbm-data"]}
    assert len(status["gpus"]) == 4
    json.loads(registry.status_json())  # still serialisable


def test_deep_verdict_survives_plain_cycles(four_card_agent, monkeypatch):
    """A bandwidth-only cycle after a deep run must not put the card with
    the data error back into service."""
    client, agent = four_card_agent
    monkeypatch.setattr(NodeAgent, "self_test", _fake_self_test)
    monkeypatch.setattr(NodeAgent, "health_check",
                        lambda self, mib=256, iters=5: [
                            {"index": i, "hbm_gbps": 6100.0, "healthy": True}
                            for i in range(4)])
    agent.publish_with_health(deep=True)
    out = agent.publish_with_health()
    assert out["sick"] == [2]
    node = client.get_node("gpu-node")
    assert not obj.node_devices(node)[2].schedulable()
    assert obj.node_card_health(node) == {2: ["hbm-data"]}


def test_publish_default_is_the_bandwidth_gate(four_card_agent, monkeypatch):
    client, agent = four_card_agent
    calls = []

    def health_check(self, mib=256, iters=5):
        calls.append((mib, iters))
        return [{"index": i, "hbm_gbps": 6100.0, "healthy": True}
                for i in range(4)]

    monkeypatch.setattr(NodeAgent, "health_check", health_check)
    monkeypatch.setattr(NodeAgent, "self_test", lambda *a, **k: pytest.fail(
        "self_test must be opt-in"))
    out = agent.publish_with_health()
    assert calls == [(256, 5)] and out["sick"] == []
    node = client.get_node("gpu-node")
    assert t.ANNOTATION_NODE_HEALTH not in node["metadata"]["annotations"]
    assert obj.node_card_health(node) == {}
    assert set(out) == {"published", "sick"}


def test_status_has_no_unhealthy_key_without_annotation(cluster):
    from tests.conftest import make_pod

    client, registry, _ = cluster
    sch = registry.default
    sch.assume(["node-a"], client.create_pod(make_pod("p", core=10)))
    assert "unhealthy_cards" not in sch.status()["nodes"]["node-a"]


@pytest.mark.parametrize("raw", ["", "not json", "[]", '{"cards": 3}',
                                 '{"cards": [{"index": "x"}]}',
                                 '{"cards": [{"index": 1, "healthy": false}]}'])
def test_node_card_health_malformed_is_empty(raw):
    node = {"metadata": {"annotations": {t.ANNOTATION_NODE_HEALTH: raw}}}
    assert obj.node_card_health(node) == {}
    assert obj.node_card_health({"metadata": {}}) == {}


def test_sick_card_search_skips_index():
    devs = [core.Device() for _ in range(4)]
    devs[2] = core.Device(core_total=0, core_avail=0, mem_total=0, mem_avail=0)
    feasible, option, _ = core.search_placement(
        devs, [core.GPUUnit(gpu_count=3)], "binpack")
    assert feasible and sorted(option.allocated[0]) == [0, 1, 3]


# --- command line ----------------------------------------------------------

def test_agent_parser_self_test_flags():
    from elastic_gpu_scheduler_amd.cmd.agent_main import build_parser

    p = build_parser()
    d = p.parse_args([])
    assert d.self_test is False and d.self_test_every == 12
    assert d.health_check is False and d.interval == 300.0
    assert d.source == "auto" and d.dry_run is False
    a = p.parse_args(["--self-test", "--self-test-every", "3"])
    assert a.self_test is True and a.self_test_every == 3
    assert p.parse_args(["--health-check"]).self_test is False


def test_agent_main_runs_deep_first_then_every_nth(monkeypatch):
    from elastic_gpu_scheduler_amd.cmd import agent_main
    from elastic_gpu_scheduler_amd.k8s import client as kc

    modes = []

    class Stop(Exception):
        pass

    def publish_with_health(self, mib=256, iters=5, deep=False):
        modes.append(deep)
        return {"published": {}, "sick": []}

    def sleep(_):
        if len(modes) >= 7:
            raise Stop

    monkeypatch.setattr(NodeAgent, "publish_with_health", publish_with_health)
    monkeypatch.setattr(kc.RealKubeClient, "from_env",
                        classmethod(lambda cls: FakeKubeClient()))
    monkeypatch.setattr(agent_main.time, "sleep", sleep)
    with pytest.raises(Stop):
        agent_main.main(["--node", "n", "--self-test", "--self-test-every", "3",
                         "--interval", "1"])
    assert modes == [True, False, False, True, False, False, True]
