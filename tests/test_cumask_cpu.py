"""gpu-core enforcement, the parts that need no GPU: the CU-mask planner, the
mask spelling, pod annotations -> container environment, the agent's
assign/sync/release cycle on a fake apiserver, and the probe's argument
checks."""
from __future__ import annotations

import json
import random

import pytest

from elastic_gpu_scheduler_amd._native import gpuprobe, gpuprobe_available
from elastic_gpu_scheduler_amd.agent.agent import NodeAgent
from elastic_gpu_scheduler_amd.agent.cumask import (CardMaskPlan, MaskGrant,
                                                    mask_hex, parse_mask_hex,
                                                    popcount)
from elastic_gpu_scheduler_amd.agent.wiring import container_wiring, pod_cu_masks
from elastic_gpu_scheduler_amd.k8s import objects as obj
from elastic_gpu_scheduler_amd.k8s.client import FakeKubeClient
from elastic_gpu_scheduler_amd.scheduler.service import GPUUnitScheduler
from elastic_gpu_scheduler_amd.utils import types as t
from tests.conftest import make_node, make_pod

needs_probe = pytest.mark.skipif(not gpuprobe_available(),
                                 reason="_gpuprobe extension not built")

FULL = (1 << 256) - 1


def granules_of(mask: int, granule: int = 8) -> list:
    """Granule indexes of a mask; asserts it is whole granules."""
    out = []
    g = 0
    while mask >> (g * granule):
        part = (mask >> (g * granule)) & ((1 << granule) - 1)
        assert part in (0, (1 << granule) - 1), hex(mask)
        if part:
            out.append(g)
        g += 1
    return out


def thirds_plan():
    plan = CardMaskPlan(256, 8)
    return plan, [plan.allocate(k, c) for k, c in
                  (("a", 50), ("b", 25), ("c", 25))]


# --- planner ---------------------------------------------------------------

def test_plan_50_25_25_is_disjoint_and_covers_the_card():
    plan, (a, b, c) = thirds_plan()
    assert plan.granules == 32
    assert [g.cus for g in (a, b, c)] == [128, 64, 64]
    assert all(g.cus == popcount(g.mask) and not g.shared for g in (a, b, c))
    assert a.mask & b.mask == a.mask & c.mask == b.mask & c.mask == 0
    assert a.mask | b.mask | c.mask == FULL
    assert granules_of(a.mask) == list(range(16))
    assert granules_of(b.mask) == list(range(16, 24))
    assert granules_of(c.mask) == list(range(24, 32))
    assert all(plan.whole_granules(g.mask) for g in (a, b, c))
    assert plan.grants() == {"a": a, "b": b, "c": c}


def test_plan_minimum_is_one_granule_and_100_is_the_card():
    plan = CardMaskPlan(256, 8)
    tiny = plan.allocate("tiny", 3)
    assert tiny == MaskGrant(mask=0xFF, cus=8, shared=False)
    assert CardMaskPlan(256, 8).allocate("zero", 0).cus == 8
    for core in (100, 250):
        whole = CardMaskPlan(256, 8).allocate("w", core)
        assert whole.mask == FULL and whole.cus == 256 and not whole.shared


def test_plan_release_and_reuse_moves_nobody():
    plan, (a, b, c) = thirds_plan()
    plan.release("b")
    d = plan.allocate("d", 10)
    assert plan.grants()["a"] == a and plan.grants()["c"] == c
    assert granules_of(d.mask) == [16, 17, 18] and not d.shared
    assert d.mask & b.mask == d.mask
    # core=30 is 9 granules; 50 + 25 + 10 + 30 oversubscribes the card, so
    # only granules 19..23 are free and the rest are shared with the tenant
    # of the least-held, lowest granules. Non-contiguous, still whole
    # granules, and its bits straddle 32-bit words.
    e = plan.allocate("e", 30)
    assert granules_of(e.mask) == [0, 1, 2, 3, 19, 20, 21, 22, 23]
    assert e.cus == 72 and e.shared
    assert plan.whole_granules(e.mask)
    assert plan.grants()["a"] == a and plan.grants()["c"] == c
    assert plan.grants()["d"] == d
    # an allocate for a held key returns the held grant
    assert plan.allocate("a", 10) == a
    plan.release("nobody")


def test_plan_fragmented_grant_within_capacity_is_unshared():
    plan = CardMaskPlan(256, 8)
    q = [plan.allocate(i, 25) for i in range(4)]
    plan.release(0)
    plan.release(2)
    e = plan.allocate("e", 30)
    assert granules_of(e.mask) == list(range(8)) + [16]
    assert not e.shared and e.mask & (q[1].mask | q[3].mask) == 0


def test_plan_oversubscribed_by_tiny_tenants_shares_never_fails():
    plan = CardMaskPlan(256, 8)
    grants = [plan.allocate(i, 2) for i in range(40)]
    assert all(g.cus == 8 for g in grants)
    first = grants[:32]
    assert not any(g.shared for g in first)
    union = 0
    for g in first:
        assert union & g.mask == 0
        union |= g.mask
    assert union == FULL
    assert all(g.shared for g in grants[32:])
    # the shared ones spread over the least-held granules
    assert [granules_of(g.mask) for g in grants[32:]] == [[i] for i in range(8)]


def test_plan_single_xcd_partition():
    plan = CardMaskPlan(32, 1)
    assert plan.granules == 32
    a, b = plan.allocate("a", 50), plan.allocate("b", 3)
    assert a.mask == 0xFFFF and b.mask == 0x10000 and b.cus == 1
    with pytest.raises(ValueError):
        CardMaskPlan(30, 8)


def test_plan_restore_reproduces_the_plan():
    plan, _ = thirds_plan()
    plan.release("b")
    plan.allocate("d", 10)
    plan.allocate("e", 30)
    again = CardMaskPlan(256, 8).restore(plan.grants())
    assert again.grants() == plan.grants()
    assert again._holders == plan._holders
    # and goes on exactly as the original would
    assert again.allocate("f", 5) == plan.allocate("f", 5)
    # restored masks are taken as they are, overlaps included
    odd = CardMaskPlan(256, 8).restore({"x": MaskGrant(0xFF, 8, False),
                                        "y": MaskGrant(0x0F, 4, False)})
    assert odd.grants()["y"].mask == 0x0F and odd._holders[0] == 2
    assert not odd.whole_granules(0x0F)
    with pytest.raises(ValueError):
        CardMaskPlan(32, 1).restore({"x": MaskGrant(1 << 32, 1, False)})


@pytest.mark.parametrize("seed", range(5))
def test_plan_random_sequences_keep_the_invariants(seed):
    rng = random.Random(seed)
    cus, granule = rng.choice([(256, 8), (32, 1), (64, 2)])
    plan = CardMaskPlan(cus, granule)
    held = {}
    for step in range(300):
        if held and rng.random() < 0.4:
            key = rng.choice(sorted(held))
            plan.release(key)
            del held[key]
        else:
            core = rng.choice([1, 2, 5, 10, 25, 30, 50, 99, 100])
            held[step] = plan.allocate(step, core)
            g = held[step]
            want = min(plan.granules, max(1, core * plan.granules // 100))
            assert g.cus == popcount(g.mask) == want * granule
            assert plan.whole_granules(g.mask)
        assert plan.grants() == held  # no held mask ever changes
        unshared = [g.mask for g in held.values() if not g.shared]
        union = 0
        for m in unshared:
            assert union & m == 0
            union |= m
    for key in list(held):
        plan.release(key)
    assert plan._holders == [0] * plan.granules


# --- mask spelling ---------------------------------------------------------

@pytest.mark.parametrize("mask", [1, 0xFF, 1 << 31, 1 << 32, 0xFF << 28,
                                  (1 << 64) | 1, 0xFF << 60, FULL,
                                  ((1 << 40) - 1) << 152])
def test_mask_hex_roundtrip(mask):
    text = mask_hex(mask)
    assert text.startswith("0x") and text == text.lower()
    assert parse_mask_hex(text) == mask
    assert parse_mask_hex(text[2:].upper()) == mask


def test_mask_hex_rejects_garbage():
    for bad in ("", "0x", "xyz", "-0x1", "0x12g"):
        with pytest.raises(ValueError):
            parse_mask_hex(bad)
    with pytest.raises(ValueError):
        mask_hex(-1)


# --- wiring and agent ------------------------------------------------------

LAYOUT = {"cus": 256, "xccs": 8, "granule": 8, "interleaved": True, "lost": []}


def stub_layouts(monkeypatch, layout=LAYOUT, cards=8):
    monkeypatch.setattr(NodeAgent, "mask_layouts",
                        lambda self: {i: dict(layout) for i in range(cards)})


@pytest.fixture
def bound():
    """A fractional two-container pod and a whole-card pod bound by the real
    scheduler."""
    client = FakeKubeClient()
    client.add_node(make_node("gpu-node"))
    sch = GPUUnitScheduler(client)
    frac = client.create_pod(make_pod(
        "frac", per_container=[{"core": 50, "memory": 2**30},
                               {"core": 25, "memory": 2**30}]))
    whole = client.create_pod(make_pod("whole", core=200))
    for pod in (frac, whole):
        ok, failed = sch.assume(["gpu-node"], pod)
        assert ok == ["gpu-node"], failed
        sch.bind("gpu-node", pod)
    return client


def test_assign_masks_wires_the_containers(bound, monkeypatch):
    stub_layouts(monkeypatch)
    agent = NodeAgent("gpu-node", bound)
    frac = bound.get_pod("default", "frac")
    entries = agent.assign_masks(frac)
    (card0,), (card1,) = obj.parse_allocation(frac)
    assert card0 == card1  # binpack: both fractions share a card
    low, high = (1 << 128) - 1, ((1 << 64) - 1) << 128
    assert entries == {
        "c0": {"card": card0, "mask": hex(low), "cus": 128, "shared": False},
        "c1": {"card": card0, "mask": hex(high), "cus": 64, "shared": False},
    }
    # the annotation is on the pod, and the wiring follows from it alone
    stored = bound.get_pod("default", "frac")
    assert t.ANNOTATION_POD_CU_MASK == "elasticgpu.io/cu-mask"
    assert json.loads(
        stored["metadata"]["annotations"][t.ANNOTATION_POD_CU_MASK]) == entries
    assert pod_cu_masks(stored) == entries
    want = {
        "c0": {"cards": [card0], "env": {"HIP_VISIBLE_DEVICES": str(card0),
                                         "ROC_GLOBAL_CU_MASK": hex(low)}},
        "c1": {"cards": [card0], "env": {"HIP_VISIBLE_DEVICES": str(card0),
                                         "ROC_GLOBAL_CU_MASK": hex(high)}},
    }
    assert container_wiring(stored) == want
    assert container_wiring(frac, entries) == want
    # idempotent per pod uid
    assert agent.assign_masks(stored) == entries
    assert len(agent.mask_plan(card0).grants()) == 2

    whole = bound.get_pod("default", "whole")
    assert agent.assign_masks(whole) == {}
    assert t.ANNOTATION_POD_CU_MASK not in \
        bound.get_pod("default", "whole")["metadata"]["annotations"]
    wiring = container_wiring(whole)
    assert list(wiring) == ["c0"] and len(wiring["c0"]["cards"]) == 2
    assert wiring["c0"]["env"] == {"HIP_VISIBLE_DEVICES": ",".join(
        str(c) for c in wiring["c0"]["cards"])}


def test_wiring_needs_a_complete_placement():
    pod = make_pod("p", per_container=[{"core": 50}, {"core": 25}])
    assert container_wiring(pod) == {}
    pod["metadata"]["annotations"] = {
        t.ANNOTATION_EGPU_CONTAINER_PREFIX + "c0": "3"}
    assert container_wiring(pod) == {}  # c1 has no card yet
    pod["metadata"]["annotations"][t.ANNOTATION_EGPU_CONTAINER_PREFIX + "c1"] = "3"
    assert container_wiring(pod) == {
        n: {"cards": [3], "env": {"HIP_VISIBLE_DEVICES": "3"}}
        for n in ("c0", "c1")}
    # a grant recorded for another card is not applied
    other = {"c0": {"card": 4, "mask": "0xff", "cus": 8, "shared": False}}
    assert "ROC_GLOBAL_CU_MASK" not in container_wiring(pod, other)["c0"]["env"]
    pod["metadata"]["annotations"][t.ANNOTATION_POD_CU_MASK] = "not json"
    assert pod_cu_masks(pod) == {}


def test_second_agent_reproduces_masks_and_completion_frees(bound, monkeypatch):
    stub_layouts(monkeypatch)
    first = NodeAgent("gpu-node", bound)
    synced = first.sync_masks()
    frac = bound.get_pod("default", "frac")
    uid = frac["metadata"]["uid"]
    assert list(synced) == [uid]
    entries = pod_cu_masks(frac)
    assert synced[uid] == entries and set(entries) == {"c0", "c1"}
    card = entries["c0"]["card"]

    # A restarted agent over the same apiserver: the same masks, read back
    # from the annotation, and later pods are planned around them.
    second = NodeAgent("gpu-node", bound)
    rv = frac["metadata"]["resourceVersion"]
    assert second.sync_masks() == synced
    assert bound.get_pod("default", "frac")["metadata"]["resourceVersion"] == rv
    assert second.mask_plan(card).grants() == first.mask_plan(card).grants()
    assert NodeAgent("other-node", bound).sync_masks() == {}

    sch = GPUUnitScheduler(bound)
    late = bound.create_pod(make_pod("late", core=10))
    ok, failed = sch.assume(["gpu-node"], late)
    assert ok == ["gpu-node"], failed
    sch.bind("gpu-node", late)
    after = second.sync_masks()
    late_entry = pod_cu_masks(bound.get_pod("default", "late"))["c0"]
    assert after[late["metadata"]["uid"]] == {"c0": late_entry}
    if late_entry["card"] == card:
        taken = parse_mask_hex(entries["c0"]["mask"]) | \
            parse_mask_hex(entries["c1"]["mask"])
        assert parse_mask_hex(late_entry["mask"]) & taken == 0
        assert granules_of(parse_mask_hex(late_entry["mask"])) == [24, 25, 26]

    # Completing the pod frees its granules at the next sync.
    bound.set_pod_phase("default", "frac", "Succeeded")
    left = second.sync_masks()
    assert uid not in left and late["metadata"]["uid"] in left
    assert all(k.startswith(late["metadata"]["uid"])
               for k in second.mask_plan(card).grants())
    again = second.mask_plan(card).allocate("next", 50)
    assert granules_of(again.mask) == list(range(16)) and not again.shared
    # a pod that is gone is released too
    bound.delete_pod("default", "late")
    assert second.sync_masks() == {}
    second.release_masks("never-seen")


def test_unsupported_layout_plans_no_masks(bound, monkeypatch):
    stub_layouts(monkeypatch, {**LAYOUT, "interleaved": False})
    agent = NodeAgent("gpu-node", bound)
    assert agent.sync_masks() == {}
    frac = bound.get_pod("default", "frac")
    assert agent.assign_masks(frac) == {}
    assert t.ANNOTATION_POD_CU_MASK not in frac["metadata"]["annotations"]
    assert agent.mask_plan(0) is None
    assert "ROC_GLOBAL_CU_MASK" not in container_wiring(frac)["c0"]["env"]
    # verify_masks launches nothing on such a card
    import elastic_gpu_scheduler_amd._native as native

    class NoLaunch:
        def cu_occupancy(self, *a, **k):
            pytest.fail("masked launch on a card with an unsupported layout")

    monkeypatch.setattr(native, "_gpuprobe", NoLaunch())
    monkeypatch.setattr(native, "_gpuprobe_tried", True)
    assert agent.verify_masks(0) == {"ok": False, "reason": "unsupported-layout"}


def test_verify_masks_judges_what_the_probe_saw(monkeypatch):
    """Over a fake probe that follows the interleaved layout, with one
    grant's queue leaking onto a neighbour's CU."""
    import elastic_gpu_scheduler_amd._native as native

    stub_layouts(monkeypatch)

    class FakeProbe:
        leak = None

        def cu_occupancy(self, device, mask=None):
            bits = [i for i in range(256) if mask >> i & 1]
            cus = {(i % 8, (i // 8) % 4, 0, i // 32) for i in bits}
            if self.leak and mask == self.leak[0]:
                cus.add(self.leak[1])
            return {"cus": [{"xcc": x, "se": s, "sh": h, "cu": c, "workgroups": 1}
                            for x, s, h, c in sorted(cus)],
                    "workgroups": len(cus), "applied_mask": mask, "seconds": 1e-4}

    fake = FakeProbe()
    monkeypatch.setattr(native, "_gpuprobe", fake)
    monkeypatch.setattr(native, "_gpuprobe_tried", True)
    agent = NodeAgent("n")
    plan = agent.mask_plan(0)
    a, b = plan.allocate("a", 50), plan.allocate("b", 25)
    report = agent.verify_masks(0)
    assert report["ok"] and report["overlaps"] == []
    assert report["per_grant"]["a"]["per_xcc"] == {x: 16 for x in range(8)}
    assert report["per_grant"]["b"]["cus"] == 64

    fake.leak = (b.mask, (0, 0, 0, 0))  # a CU of grant a
    report = agent.verify_masks(0)
    assert not report["ok"] and not report["per_grant"]["b"]["ok"]
    assert report["overlaps"] == [{"a": "a", "b": "b", "cus": [(0, 0, 0, 0)]}]
    # a recorded mask that is not whole granules is never launched
    fake.leak = None
    plan.restore({"odd": MaskGrant(0x0F << 200, 4, False)})
    report = agent.verify_masks(0)
    assert report["per_grant"]["odd"] == {"ok": False,
                                          "reason": "not-whole-granules"}
    assert not report["ok"] and report["per_grant"]["a"]["ok"]


def test_agent_parser_cu_mask_flags():
    from elastic_gpu_scheduler_amd.cmd.agent_main import build_parser

    p = build_parser()
    d = p.parse_args([])
    assert d.cu_masks is False and d.cu_mask_layout is False
    assert p.parse_args(["--cu-masks"]).cu_masks is True
    assert p.parse_args(["--cu-mask-layout"]).cu_mask_layout is True


def test_agent_main_syncs_masks_only_when_asked(monkeypatch):
    from elastic_gpu_scheduler_amd.cmd import agent_main
    from elastic_gpu_scheduler_amd.k8s import client as kc

    calls = []
    monkeypatch.setattr(NodeAgent, "publish", lambda self: calls.append("publish"))
    monkeypatch.setattr(NodeAgent, "sync_masks",
                        lambda self: calls.append("sync") or {})
    monkeypatch.setattr(kc.RealKubeClient, "from_env",
                        classmethod(lambda cls: FakeKubeClient()))
    assert agent_main.main(["--node", "n", "--interval", "0"]) == 0
    assert calls == ["publish"]
    assert agent_main.main(["--node", "n", "--interval", "0", "--cu-masks"]) == 0
    assert calls == ["publish", "publish", "sync"]


def test_agent_main_prints_layouts(monkeypatch, capsys):
    from elastic_gpu_scheduler_amd.cmd import agent_main

    stub_layouts(monkeypatch, cards=2)
    assert agent_main.main(["--cu-mask-layout"]) == 0
    assert json.loads(capsys.readouterr().out) == {"0": LAYOUT, "1": LAYOUT}


# --- binding argument checks -----------------------------------------------

@needs_probe
def test_probe_rejects_bad_masks_before_touching_the_device():
    p = gpuprobe()
    for bad in (0, -1, 1 << 300, 1 << 256):
        with pytest.raises(ValueError):
            p.cu_occupancy(0, mask=bad)
        with pytest.raises(ValueError):
            p.cu_mask_throughput(0, mask=bad)
    with pytest.raises(TypeError):
        p.cu_occupancy(0, mask="0xff")


@needs_probe
def test_cumask_probes_raise_without_device():
    import torch

    if torch.cuda.is_available():
        return  # a device is visible: covered by the gpu-marked tests
    p = gpuprobe()
    with pytest.raises(RuntimeError):
        p.cu_occupancy(0)
    with pytest.raises(RuntimeError):
        p.cu_occupancy(0, mask=0xFF)
    with pytest.raises(RuntimeError):
        p.cu_mask_layout(0)
    with pytest.raises(RuntimeError):
        p.cu_mask_throughput(0, mask=0xFF, iters=16)
