"""The two-tenant interference probe, the parts that need no GPU: overlap of
stamped launches, the parent's handling of (fake) children, the report's
arithmetic and its refusal to go on after a failed child, the child entry
over a fake probe, the agent's gate, the CLI flag, and the probe's argument
checks."""
from __future__ import annotations

import io
import json
import subprocess
import threading

import pytest

from elastic_gpu_scheduler_amd._native import gpuprobe, gpuprobe_available
from elastic_gpu_scheduler_amd.agent import cotenancy
from elastic_gpu_scheduler_amd.agent.agent import NodeAgent
from elastic_gpu_scheduler_amd.agent.cotenancy import (isolation_report, overlap,
                                                       run_pair)
from elastic_gpu_scheduler_amd.agent.cumask import mask_hex, popcount
from elastic_gpu_scheduler_amd.agent.wiring import ENV_CU_MASK

needs_probe = pytest.mark.skipif(not gpuprobe_available(),
                                 reason="_gpuprobe extension not built")

LAYOUT = {"cus": 256, "xccs": 8, "granule": 8, "interleaved": True, "lost": []}
LOW, HIGH = (1 << 128) - 1, ((1 << 128) - 1) << 128
CHECKSUM = 0x1234ABCD
BYTES = 1 << 20


def spans(*pairs):
    return [{"t0": a, "t1": b} for a, b in pairs]


# --- overlap ----------------------------------------------------------------

def test_overlap_disjoint_is_solo():
    got = overlap(spans((0, 100), (200, 300)), spans((100, 200), (300, 400)))
    assert got == [{"fraction": 0.0, "label": "solo"}] * 2


def test_overlap_across_a_gap_free_union_is_contended():
    b = spans((50, 100), (0, 50), (100, 150))  # unsorted on purpose
    got = overlap(spans((10, 140), (0, 150)), b)
    assert got == [{"fraction": 1.0, "label": "contended"}] * 2


def test_overlap_either_side_of_the_line():
    b = spans((0, 1000))
    below, above, exact = overlap(
        spans((60, 1060), (40, 1040), (50, 1050)), b)
    assert below == {"fraction": 0.94, "label": "mixed"}
    assert above == {"fraction": 0.96, "label": "contended"}
    assert exact == {"fraction": 0.95, "label": "contended"}


def test_overlap_with_a_gap_in_b():
    b = spans((0, 400), (600, 1000))
    (got,) = overlap(spans((0, 1000)), b)
    assert got == {"fraction": 0.8, "label": "mixed"}
    # a gap of 1 % of the launch does not disqualify it
    (got,) = overlap(spans((0, 1000)), spans((0, 495), (505, 1000)))
    assert got["label"] == "contended" and got["fraction"] == 0.99
    # overlapping intervals of B are not counted twice
    (got,) = overlap(spans((0, 1000)), spans((0, 300), (200, 500)))
    assert got == {"fraction": 0.5, "label": "mixed"}


def test_overlap_empty_lists_and_empty_intervals():
    assert overlap([], []) == []
    assert overlap([], spans((0, 10))) == []
    assert overlap(spans((0, 10)), []) == [{"fraction": 0.0, "label": "solo"}]
    assert overlap(spans((5, 5)), spans((0, 10))) == [
        {"fraction": 0.0, "label": "mixed"}]
    assert overlap(spans((0, 10)), spans((7, 7))) == [
        {"fraction": 0.0, "label": "solo"}]


# --- fake children ----------------------------------------------------------

class FakeChild:
    """Speaks the child protocol: READY, waits for GO, then its ending."""

    def __init__(self, argv, env, result=None, code=0, hang=False):
        self.argv, self.env = list(argv), dict(env)
        self.kind = argv[argv.index("--kind") + 1]
        self.launches = int(argv[argv.index("--launches") + 1])
        self.result, self.code, self.hang = result, code, hang
        self.returncode = None
        self.killed = False
        self._go, self._gone = threading.Event(), threading.Event()
        self.stdin = self
        self.stdout = self._lines()

    def write(self, text):
        if text.strip() == "GO":
            self._go.set()

    def flush(self):
        pass

    def _lines(self):
        yield "noise before the handshake\n"
        yield "READY\n"
        self._go.wait(30)
        if self.hang:
            self._gone.wait(30)  # until killed
            return
        if self.result is not None:
            yield "TENANT " + json.dumps(self.result) + "\n"
        self.returncode = self.code
        self._gone.set()

    def poll(self):
        return self.returncode

    def wait(self, timeout=None):
        if not self._gone.wait(timeout):
            raise subprocess.TimeoutExpired("fake-child", timeout)
        return self.returncode

    def kill(self):
        self.killed = True
        if self.returncode is None:
            self.returncode = -9
        self._gone.set()
        self._go.set()


def tenant_result(kind, launches, checksum=CHECKSUM):
    """launches: [(t0, t1, rate)]."""
    out = {"kind": kind, "applied_mask": None, "tick_hz": 1e8,
           "workgroups": 4096, "work_per_launch": 1e9,
           "launches": [{"t0": a, "t1": b, "seconds": (b - a) / 1e8,
                         "event_seconds": (b - a) / 1e8 * 1.01, "rate": r}
                        for a, b, r in launches]}
    rates = sorted(r for _, _, r in launches)
    out["rate"] = rates[len(rates) // 2]
    if kind == "stream":
        out.update(bytes=BYTES, passes=3, checksum=checksum)
    else:
        out["iters"] = 64
    return out


def steady(kind, start, n, rate, length=1000, **kw):
    return tenant_result(
        kind, [(start + i * length, start + (i + 1) * length - 1, rate)
               for i in range(n)], **kw)


class Spawner:
    """spawn() for run_pair: child n is made by script(n, argv, env)."""

    def __init__(self, script):
        self.script = script
        self.log = []

    def __call__(self, argv, env):
        child = self.script(len(self.log), argv, env)
        self.log.append(child)
        return child


SOLO_RATE = {"fma": 100.0, "stream": 40.0}


def well_behaved(n, argv, env, **overrides):
    """Children 0..3 are the solo runs; later ones come in pairs whose first
    tenant is slowed to 0.5 and whose second to 0.8 while they overlap."""
    kind = argv[argv.index("--kind") + 1]
    count = int(argv[argv.index("--launches") + 1])
    if n < 4:
        return FakeChild(argv, env, steady(kind, 10_000 * n, count, SOLO_RATE[kind],
                                           **overrides))
    base = SOLO_RATE[kind]
    if n % 2 == 0:
        # starts 300 ticks before the neighbour: one mixed launch with a
        # wild rate, then contended ones, then two solo after its end
        launches = [(99_700, 100_699, base * 7)]
        launches += [(100_700 + 1000 * i, 101_699 + 1000 * i, base * 0.5)
                     for i in range(count - 3)]
        end = 100_700 + 1000 * (count - 3)
        launches += [(end + 5000, end + 5999, base), (end + 6000, end + 6999, base)]
        return FakeChild(argv, env, tenant_result(kind, launches, **overrides))
    return FakeChild(argv, env, steady(kind, 100_000, count, base * 0.8, **overrides))


TENANTS = [{"mask": LOW}, {"mask": HIGH}]


def expected(seed, nbytes):
    assert (seed, nbytes) == (1, BYTES)
    return CHECKSUM


def test_run_pair_handshake_and_environment():
    spawn = Spawner(well_behaved)
    out = run_pair(3, [{"mask": LOW, "kind": "fma"}, {"mask": HIGH, "kind": "stream"}],
                   launches=5, iters=64, bytes=BYTES, passes=3, seed=9, spawn=spawn)
    assert out["ok"] and [r["kind"] for r in out["tenants"]] == ["fma", "stream"]
    a, b = spawn.log
    assert a.env[ENV_CU_MASK] == mask_hex(LOW) and b.env[ENV_CU_MASK] == mask_hex(HIGH)
    assert a.argv[1:4] == ["-m", "elastic_gpu_scheduler_amd.agent.cotenancy", "--child"]
    for flag, value in (("--device", "3"), ("--launches", "5"), ("--iters", "64"),
                        ("--bytes", str(BYTES)), ("--passes", "3"), ("--seed", "9")):
        assert a.argv[a.argv.index(flag) + 1] == value
    assert not a.killed and not b.killed
    # `kinds` names the kinds instead; a tenant may carry its own launches
    spawn = Spawner(well_behaved)
    out = run_pair(0, [{"mask": LOW, "kind": "fma", "launches": 11}], ["stream"],
                   spawn=spawn)
    assert out["ok"] and spawn.log[0].kind == "stream" and spawn.log[0].launches == 11
    with pytest.raises(ValueError):
        run_pair(0, [], spawn=spawn)
    with pytest.raises(ValueError):
        run_pair(0, [{"mask": 1, "kind": "fma"}] * 3, spawn=spawn)


def test_report_ratios_come_from_the_contended_launches_only():
    spawn = Spawner(well_behaved)
    report = isolation_report(0, TENANTS, launches=8, bytes=BYTES, spawn=spawn,
                              expected_checksum=expected)
    assert report["ok"] and "reason" not in report
    assert [c.kind for c in spawn.log] == [
        "fma", "stream", "fma", "stream",  # solo: tenant 0, then tenant 1
        "fma", "fma", "stream", "stream", "fma", "stream", "stream", "fma"]
    assert [c.env[ENV_CU_MASK] for c in spawn.log[:4]] == [
        mask_hex(LOW)] * 2 + [mask_hex(HIGH)] * 2
    assert [c.env[ENV_CU_MASK] for c in spawn.log[4:]] == [
        mask_hex(LOW), mask_hex(HIGH)] * 4
    assert report["solo"][0]["fma"]["rate"] == 100.0
    assert report["solo"][1]["stream"] == {"rate": 40.0, "seconds": 999 / 1e8,
                                           "launches": 8, "workgroups": 4096}
    assert list(report["pairs"]) == ["fma/fma", "stream/stream", "fma/stream",
                                     "stream/fma"]
    for name, pair in report["pairs"].items():
        kinds = name.split("/")
        first, second = pair["tenants"]
        assert pair["ok"] and [first["kind"], second["kind"]] == kinds
        # 8 launches: 1 mixed (rate x7), 5 contended (x0.5), 2 solo (x1)
        assert first["launches"] == 8 and first["contended_launches"] == 5
        assert first["mixed_launches"] == 1 and first["solo_launches"] == 2
        assert first["solo_rate"] == SOLO_RATE[kinds[0]]
        assert first["contended_rate"] == SOLO_RATE[kinds[0]] * 0.5
        assert first["ratio"] == 0.5
        # the neighbour runs 100000..107999: its launch 5 is covered to 0.7
        # only and launches 6, 7 fall into the first tenant's pause
        assert second["contended_launches"] == 5 and second["ratio"] == 0.8


def test_report_balances_unequal_tenants_by_launch_count():
    def script(n, argv, env):
        kind = argv[argv.index("--kind") + 1]
        count = int(argv[argv.index("--launches") + 1])
        length = 4000 if n in (0, 2) else 1000  # tenant 0 is four times slower
        return FakeChild(argv, env, steady(kind, 50_000, count, 10.0, length=length))

    spawn = Spawner(script)
    report = isolation_report(0, TENANTS, pairs=[("fma", "fma")], launches=6,
                              spawn=spawn)
    assert [c.launches for c in spawn.log] == [6, 6, 6, 50]  # ceil(2 * 6 * 3999 / 999) + 1
    first, second = report["pairs"]["fma/fma"]["tenants"]
    assert report["ok"] and first["contended_launches"] == 6
    assert second["contended_launches"] == 24 and second["solo_launches"] == 26
    assert cotenancy._balanced(8, [1.0, 1.2]) == [8, 8]
    assert cotenancy._balanced(8, [1.0, 100.0]) == [64, 8]


def test_report_needs_three_contended_launches():
    def script(n, argv, env):
        kind = argv[argv.index("--kind") + 1]
        if n == 5:  # overlaps only the neighbour's first two launches
            return FakeChild(argv, env, steady(kind, 100_700, 2, 80.0))
        return well_behaved(n, argv, env)

    report = isolation_report(0, TENANTS, launches=8, bytes=BYTES,
                              spawn=Spawner(script), expected_checksum=expected)
    first, second = report["pairs"]["fma/fma"]["tenants"]
    assert not report["ok"] and report["reason"] == "no-overlap"
    assert all(report["pairs"][name]["ok"]
               for name in ("stream/stream", "fma/stream", "stream/fma"))
    assert first["contended_launches"] == 2 and first["reason"] == "no-overlap"
    assert "ratio" not in first and "contended_rate" not in first
    assert second["contended_launches"] == 2 and "ratio" not in second
    assert report["pairs"]["fma/fma"]["ok"] is False


def test_report_wrong_checksum_is_not_ok():
    def script(n, argv, env):
        if n == 7:  # second tenant of stream/stream
            return well_behaved(n, argv, env, checksum=CHECKSUM ^ 1)
        return well_behaved(n, argv, env)

    report = isolation_report(0, TENANTS, launches=8, bytes=BYTES,
                              spawn=Spawner(script), expected_checksum=expected)
    assert not report["ok"] and report["reason"] == "bad-checksum"
    pair = report["pairs"]["stream/stream"]
    assert not pair["ok"] and pair["tenants"][1]["reason"] == "bad-checksum"
    assert "reason" not in pair["tenants"][0]
    assert report["pairs"]["fma/fma"]["ok"]
    # a solo run's checksum counts too
    spawn = Spawner(lambda n, argv, env: well_behaved(
        n, argv, env, **({"checksum": 5} if n == 1 else {})))
    report = isolation_report(0, TENANTS, launches=8, bytes=BYTES, spawn=spawn,
                              expected_checksum=expected)
    assert not report["ok"] and report["reason"] == "bad-checksum"


def test_failed_child_ends_the_report_and_its_sibling():
    def script(n, argv, env):
        if n == 4:  # first tenant of the first pair: dies of a segfault after GO
            return FakeChild(argv, env, result=None, code=-11)
        if n == 5:
            return FakeChild(argv, env, hang=True)
        return well_behaved(n, argv, env)

    spawn = Spawner(script)
    report = isolation_report(0, TENANTS, launches=8, bytes=BYTES, spawn=spawn,
                              expected_checksum=expected)
    assert report["ok"] is False and report["reason"] == "child-failed"
    assert report["detail"]["tenant"] == 0 and report["detail"]["returncode"] == -11
    assert len(spawn.log) == 6  # nothing was started after it
    assert spawn.log[5].killed and not spawn.log[4].killed
    assert report["pairs"] == {"fma/fma": {"ok": False, "reason": "child-failed"}}
    # a failing solo run stops everything too
    spawn = Spawner(lambda n, argv, env: FakeChild(argv, env, result=None, code=1))
    report = isolation_report(0, TENANTS, spawn=spawn)
    assert report["reason"] == "child-failed" and len(spawn.log) == 1
    assert report["pairs"] == {}


def test_child_exceeding_its_timeout_is_killed():
    spawn = Spawner(lambda n, argv, env: FakeChild(argv, env, hang=True))
    out = run_pair(0, [{"mask": LOW, "kind": "fma"}], timeout=0.05, spawn=spawn)
    assert out["ok"] is False and out["reason"] == "child-failed"
    assert "timed out" in out["detail"]["what"] and spawn.log[0].killed


# --- child entry ------------------------------------------------------------

def test_child_entry_says_ready_before_reading_go(monkeypatch):
    import elastic_gpu_scheduler_amd._native as native

    calls = []
    out = io.StringIO()

    class FakeProbe:
        def cu_tenant_run(self, device, mask, **kw):
            calls.append((device, mask, kw))
            return steady(kw["kind"], 0, kw["launches"], 1.0)

    class Stdin(io.StringIO):
        def readline(self):
            assert out.getvalue() == "READY\n"  # and one warm-up call so far
            assert len(calls) == 1
            return super().readline()

    monkeypatch.setattr(native, "_gpuprobe", FakeProbe())
    monkeypatch.setattr(native, "_gpuprobe_tried", True)
    argv = ["--child", "--device", "2", "--kind", "stream", "--launches", "5",
            "--bytes", "4096", "--passes", "3", "--seed", "7"]
    assert cotenancy.child_main(argv, stdin=Stdin("GO\n"), stdout=out) == 0
    window = {"kind": "stream", "iters": 0, "bytes": 4096, "passes": 3, "seed": 7}
    assert calls == [(2, None, {"launches": 1, **window}),
                     (2, None, {"launches": 5, **window})]
    lines = out.getvalue().splitlines()
    assert lines[0] == "READY" and len(lines) == 2
    assert [ln for ln in lines if ln.startswith("TENANT ")] == [lines[1]]
    assert json.loads(lines[1][len("TENANT "):]) == steady("stream", 0, 5, 1.0)
    # anything but GO: no measured run, no TENANT line
    out.seek(0)
    out.truncate()
    del calls[:]
    assert cotenancy.child_main(argv, stdin=Stdin(""), stdout=out) == 3
    assert out.getvalue() == "READY\n" and len(calls) == 1


# --- agent and CLI ----------------------------------------------------------

def stub_layouts(monkeypatch, layout=LAYOUT, cards=1):
    monkeypatch.setattr(NodeAgent, "mask_layouts",
                        lambda self: {i: dict(layout) for i in range(cards)})


def test_verify_isolation_unsupported_layout_spawns_nothing(monkeypatch):
    spawn = Spawner(well_behaved)
    for layout in ({**LAYOUT, "interleaved": False}, {}):
        stub_layouts(monkeypatch, layout)
        assert NodeAgent("n").verify_isolation(0, spawn=spawn) == {
            "ok": False, "reason": "unsupported-layout"}
    stub_layouts(monkeypatch)
    assert NodeAgent("n").verify_isolation(5, spawn=spawn)["reason"] == \
        "unsupported-layout"  # no such card
    out = NodeAgent("n").verify_isolation(0, shares=(60, 60), spawn=spawn)
    assert out["ok"] is False and out["reason"] == "shares-overlap"
    assert spawn.log == []


def test_verify_isolation_runs_planner_masks_on_a_scratch_plan(monkeypatch):
    stub_layouts(monkeypatch)
    agent = NodeAgent("n")
    live = agent.mask_plan(0)
    live.allocate("running-tenant", 25)
    spawn = Spawner(well_behaved)
    report = agent.verify_isolation(0, shares=(25, 75), launches=8, bytes=BYTES,
                                    spawn=spawn, expected_checksum=expected)
    assert report["ok"] and len(report["pairs"]) == 4
    a, b = report["tenants"]
    assert (a["core"], a["cus"], b["core"], b["cus"]) == (25, 64, 75, 192)
    ma, mb = int(a["mask"], 16), int(b["mask"], 16)
    assert ma & mb == 0 and ma | mb == (1 << 256) - 1
    assert popcount(ma) == 64 and live.whole_granules(ma) and live.whole_granules(mb)
    assert {c.env[ENV_CU_MASK] for c in spawn.log} == {a["mask"], b["mask"]}
    assert list(agent.mask_plan(0).grants()) == ["running-tenant"]


def test_agent_parser_co_tenancy_flag():
    from elastic_gpu_scheduler_amd.cmd.agent_main import build_parser

    p = build_parser()
    assert p.parse_args([]).co_tenancy is None
    assert p.parse_args(["--co-tenancy"]).co_tenancy == (50, 50)
    assert p.parse_args(["--co-tenancy", "25,75"]).co_tenancy == (25, 75)
    for bad in ("0,50", "50", "10,20,30", "a,b", "50,101"):
        with pytest.raises(SystemExit):
            p.parse_args(["--co-tenancy", bad])


def test_agent_main_reports_every_card_in_turn(monkeypatch, capsys):
    from elastic_gpu_scheduler_amd.cmd import agent_main

    stub_layouts(monkeypatch, cards=2)
    calls = []
    monkeypatch.setattr(
        NodeAgent, "verify_isolation",
        lambda self, card, shares: calls.append((card, shares)) or {"ok": True})
    assert agent_main.main(["--co-tenancy", "25,75"]) == 0
    assert calls == [(0, (25, 75)), (1, (25, 75))]
    assert json.loads(capsys.readouterr().out) == {"0": {"ok": True},
                                                   "1": {"ok": True}}


# --- binding argument checks ------------------------------------------------

@needs_probe
def test_tenant_run_rejects_bad_arguments_before_touching_the_device():
    p = gpuprobe()
    with pytest.raises(ValueError):
        p.cu_tenant_run(0, kind="x")
    with pytest.raises(ValueError):
        p.cu_tenant_run(0, mask=0xFF, kind="")
    for bad in (0, -1, 1 << 300, 1 << 256):
        for kind in ("fma", "stream"):
            with pytest.raises(ValueError):
                p.cu_tenant_run(0, mask=bad, kind=kind)
    with pytest.raises(TypeError):
        p.cu_tenant_run(0, mask="0xff")


@needs_probe
def test_tenant_run_raises_without_device():
    import torch

    if torch.cuda.is_available():
        return  # a device is visible: covered by the gpu-marked tests
    p = gpuprobe()
    for kind in ("fma", "stream"):
        with pytest.raises(RuntimeError):
            p.cu_tenant_run(0, kind=kind, launches=1, iters=16, bytes=16, passes=1)
        with pytest.raises(RuntimeError):
            p.cu_tenant_run(0, mask=0xFF, kind=kind)


@needs_probe
def test_pattern_word_is_still_the_host_oracle():
    p = gpuprobe()
    assert p.pattern_xor(1, 0, 3) == (p.pattern_word(1, 0) ^ p.pattern_word(1, 1)
                                      ^ p.pattern_word(1, 2))
