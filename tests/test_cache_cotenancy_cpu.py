"""The cache tenant of the interference probe, the parts that need no GPU:
per-tenant and per-kind windows in the parent's argv, the report's checksum
check for the new kind, the working-set sweep over (fake) children, the
agent's gate, the CLI flag, and the probe's argument checks."""
from __future__ import annotations

import json
import subprocess
import threading

import pytest

from elastic_gpu_scheduler_amd._native import gpuprobe, gpuprobe_available
from elastic_gpu_scheduler_amd.agent import cotenancy
from elastic_gpu_scheduler_amd.agent.agent import NodeAgent
from elastic_gpu_scheduler_amd.agent.cotenancy import isolation_report, run_pair
from elastic_gpu_scheduler_amd.agent.cumask import mask_hex, popcount
from elastic_gpu_scheduler_amd.agent.wiring import ENV_CU_MASK

needs_probe = pytest.mark.skipif(not gpuprobe_available(),
                                 reason="_gpuprobe extension not built")

LAYOUT = {"cus": 256, "xccs": 8, "granule": 8, "interleaved": True, "lost": []}
LOW, HIGH = (1 << 128) - 1, ((1 << 128) - 1) << 128
MIB = 1 << 20
CACHE_BYTES, STREAM_BYTES = 12 * MIB, 1 << 30
WINDOWS = {"cache": {"bytes": CACHE_BYTES, "passes": 4097},
           "stream": {"bytes": STREAM_BYTES}}
SOLO_RATE = {"fma": 100.0, "stream": 40.0, "cache": 200.0}


def checksum_of(seed, nbytes):
    """The fake oracle: any function of both will do."""
    return (seed * 1_000_003) ^ nbytes


# --- fake children ----------------------------------------------------------

def flag(argv, name):
    return argv[argv.index(name) + 1]


class FakeChild:
    """Speaks the child protocol: READY, waits for GO, then its ending."""

    def __init__(self, argv, env, result=None, code=0):
        self.argv, self.env = list(argv), dict(env)
        self.kind = flag(argv, "--kind")
        self.window = {k: int(flag(argv, "--" + k))
                       for k in ("launches", "iters", "bytes", "passes", "seed")}
        self.result, self.code = result, code
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
        yield "READY\n"
        self._go.wait(30)
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


def answer(argv, start=100_000, rate=None, wrong=False):
    """What a child given `argv` would print: `launches` back-to-back
    launches of 1000 ticks from `start`, the window it was asked for and,
    for a kind that reads a buffer, the checksum of that buffer."""
    kind = flag(argv, "--kind")
    count, nbytes = int(flag(argv, "--launches")), int(flag(argv, "--bytes"))
    rate = SOLO_RATE[kind] if rate is None else rate
    out = {"kind": kind, "applied_mask": None, "tick_hz": 1e8, "workgroups": 2048,
           "work_per_launch": 1e9, "rate": rate,
           "launches": [{"t0": start + 1000 * i, "t1": start + 1000 * i + 999,
                         "seconds": 999 / 1e8, "event_seconds": 1000 / 1e8,
                         "rate": rate} for i in range(count)]}
    if kind == "fma":
        out["iters"] = int(flag(argv, "--iters"))
    else:
        out.update(bytes=nbytes, passes=int(flag(argv, "--passes")) | 1,
                   checksum=checksum_of(int(flag(argv, "--seed")), nbytes) ^ wrong)
        if kind == "cache":
            out["bytes_per_cu"] = nbytes / 256
    return out


class Spawner:
    """spawn() for run_pair: child n is made by script(n, argv, env)."""

    def __init__(self, script=None):
        self.script = script or (lambda n, argv, env: FakeChild(argv, env, answer(argv)))
        self.log = []

    def __call__(self, argv, env):
        child = self.script(len(self.log), argv, env)
        self.log.append(child)
        return child


TENANTS = [{"mask": LOW}, {"mask": HIGH}]


# --- per-tenant windows in run_pair -----------------------------------------

def test_child_parser_accepts_the_cache_kind():
    args = cotenancy._child_parser().parse_args(
        ["--child", "--kind", "cache", "--bytes", "4096", "--passes", "5"])
    assert (args.kind, args.bytes, args.passes) == ("cache", 4096, 5)
    assert "cache" in cotenancy.KINDS
    with pytest.raises(SystemExit):
        cotenancy._child_parser().parse_args(["--child", "--kind", "cach"])


def test_run_pair_gives_a_tenant_its_own_window():
    spawn = Spawner()
    out = run_pair(1, [{"mask": LOW, "kind": "cache", "bytes": CACHE_BYTES,
                        "passes": 4097, "iters": 5},
                       {"mask": HIGH, "kind": "stream"}],
                   launches=4, iters=64, bytes=STREAM_BYTES, passes=7, seed=9,
                   spawn=spawn)
    assert out["ok"] and [r["kind"] for r in out["tenants"]] == ["cache", "stream"]
    a, b = spawn.log
    assert a.window == {"launches": 4, "iters": 5, "bytes": CACHE_BYTES,
                        "passes": 4097, "seed": 9}
    assert b.window == {"launches": 4, "iters": 64, "bytes": STREAM_BYTES,
                        "passes": 7, "seed": 9}
    assert a.env[ENV_CU_MASK] == mask_hex(LOW) and b.env[ENV_CU_MASK] == mask_hex(HIGH)
    assert out["tenants"][0]["bytes"] == CACHE_BYTES
    # a tenant that carries nothing: the argv of before, flag for flag
    spawn = Spawner()
    run_pair(3, [{"mask": LOW, "kind": "fma"}], launches=5, iters=64, bytes=MIB,
             passes=3, seed=9, spawn=spawn)
    assert spawn.log[0].argv[1:] == [
        "-m", "elastic_gpu_scheduler_amd.agent.cotenancy", "--child",
        "--device", "3", "--kind", "fma", "--launches", "5", "--iters", "64",
        "--bytes", str(MIB), "--passes", "3", "--seed", "9"]
    with pytest.raises(ValueError):
        run_pair(0, [{"mask": LOW, "kind": "cach"}], spawn=spawn)


# --- isolation_report with windows ------------------------------------------

def test_report_gives_each_kind_its_window_solo_and_paired():
    spawn = Spawner()
    asked = []

    def expected(seed, nbytes):
        asked.append(nbytes)
        return checksum_of(seed, nbytes)

    report = isolation_report(0, TENANTS, pairs=cotenancy.CACHE_PAIRS, launches=8,
                              iters=32, seed=3, windows=WINDOWS, spawn=spawn,
                              expected_checksum=expected)
    assert report["ok"], report
    assert [c.kind for c in spawn.log] == [
        "stream", "cache",          # solo, tenant 0: the kinds it has in a pair
        "fma", "stream", "cache",   # solo, tenant 1
        "cache", "cache", "cache", "stream", "stream", "cache", "cache", "fma"]
    assert list(report["pairs"]) == ["cache/cache", "cache/stream", "stream/cache",
                                     "cache/fma"]
    for c in spawn.log:
        want = {"launches": 8, "iters": 32, "bytes": 0, "passes": 0, "seed": 3}
        want.update(WINDOWS.get(c.kind, {}))
        assert c.window == want, (c.kind, c.window)
    assert [c.env[ENV_CU_MASK] for c in spawn.log[5:]] == [mask_hex(LOW),
                                                           mask_hex(HIGH)] * 4
    assert sorted(asked) == [CACHE_BYTES, STREAM_BYTES]  # once per size
    assert report["solo"][0]["cache"]["rate"] == 200.0
    assert report["solo"][1]["fma"]["rate"] == 100.0
    for pair in report["pairs"].values():
        for t in pair["tenants"]:
            assert t["contended_launches"] == 8 and t["ratio"] == 1.0


def test_report_wrong_cache_checksum_is_not_ok():
    def script(n, argv, env):  # three solo runs, then child 4: second of cache/cache
        return FakeChild(argv, env, answer(argv, wrong=(n == 4)))

    report = isolation_report(0, TENANTS, pairs=[("cache", "cache"), ("cache", "fma")],
                              windows=WINDOWS, spawn=Spawner(script),
                              expected_checksum=checksum_of)
    assert not report["ok"] and report["reason"] == "bad-checksum"
    pair = report["pairs"]["cache/cache"]
    assert not pair["ok"] and pair["tenants"][1]["reason"] == "bad-checksum"
    assert "reason" not in pair["tenants"][0]
    assert report["pairs"]["cache/fma"]["ok"]
    # a solo cache run's checksum counts too
    spawn = Spawner(lambda n, argv, env: FakeChild(argv, env, answer(argv, wrong=(n == 0))))
    report = isolation_report(0, TENANTS, pairs=[("cache", "cache")], windows=WINDOWS,
                              spawn=spawn, expected_checksum=checksum_of)
    assert not report["ok"] and report["reason"] == "bad-checksum"


def test_report_refuses_unknown_kinds_before_spawning():
    spawn = Spawner()
    for pairs in ([("cache", "cach")], [("l2", "stream")], [("cache",)]):
        with pytest.raises(ValueError):
            isolation_report(0, TENANTS, pairs=pairs, spawn=spawn)
    with pytest.raises(ValueError):
        isolation_report(0, TENANTS, windows={"cach": {"bytes": 16}}, spawn=spawn)
    with pytest.raises(ValueError):
        isolation_report(0, TENANTS, windows={"cache": {"byte": 16}}, spawn=spawn)
    assert spawn.log == []


def test_report_without_windows_sends_the_argv_of_before():
    assert cotenancy.ALL_PAIRS == (("fma", "fma"), ("stream", "stream"),
                                   ("fma", "stream"), ("stream", "fma"))
    logs = []
    for extra in ({}, {"windows": None}, {"windows": {}}):
        spawn = Spawner()
        report = isolation_report(2, TENANTS, launches=8, iters=64, bytes=MIB, passes=3,
                                  seed=5, spawn=spawn, expected_checksum=checksum_of,
                                  **extra)
        assert report["ok"]
        logs.append([c.argv[1:] for c in spawn.log])
    assert logs[0] == logs[1] == logs[2] and len(logs[0]) == 12
    for argv, kind in zip(logs[0], ["fma", "stream", "fma", "stream", "fma", "fma",
                                    "stream", "stream", "fma", "stream", "stream",
                                    "fma"]):
        assert argv == ["-m", "elastic_gpu_scheduler_amd.agent.cotenancy", "--child",
                        "--device", "2", "--kind", kind, "--launches", "8",
                        "--iters", "64", "--bytes", str(MIB), "--passes", "3",
                        "--seed", "5"]


def test_cache_passes_fills_a_launch_within_the_probes_range():
    assert cotenancy.cache_passes(12 * MIB) == (127 << 30) // (12 * MIB) | 1 == 10837
    assert cotenancy.cache_passes(128 * MIB) == 1017
    assert cotenancy.cache_passes(1 << 30, 16 << 30) == 17  # even -> odd
    assert cotenancy.cache_passes(16) == 65535 and cotenancy.cache_passes(0) == 65535
    assert cotenancy.cache_passes(1 << 30, 1) == 1


# --- cache_profile ----------------------------------------------------------

SIZES = [2 * MIB, 24 * MIB, 512 * MIB]


def test_cache_profile_one_child_per_size_in_order():
    spawn = Spawner(lambda n, argv, env: FakeChild(
        argv, env, answer(argv, rate=1000.0 / (n + 1))))
    out = cotenancy.cache_profile(1, LOW, SIZES, launches=4, seed=7, spawn=spawn,
                                  expected_checksum=checksum_of)
    assert out["ok"] and len(spawn.log) == 3
    assert [c.kind for c in spawn.log] == ["cache"] * 3
    assert [c.window["bytes"] for c in spawn.log] == SIZES
    assert [c.window["passes"] for c in spawn.log] == [8193, 683, 33]  # 16 GiB a launch
    assert all(c.window["launches"] == 4 and c.window["seed"] == 7 for c in spawn.log)
    assert all(c.env[ENV_CU_MASK] == mask_hex(LOW) for c in spawn.log)
    assert all(flag(c.argv, "--device") == "1" for c in spawn.log)
    assert out["profile"] == [
        {"bytes": size, "bytes_per_cu": size / 256, "rate": 1000.0 / (n + 1),
         "seconds": 999 / 1e8, "passes": p}
        for n, (size, p) in enumerate(zip(SIZES, [8193, 683, 33]))]
    # given passes are passed on
    spawn = Spawner()
    cotenancy.cache_profile(0, LOW, SIZES[:1], passes=5, spawn=spawn,
                            expected_checksum=checksum_of)
    assert spawn.log[0].window["passes"] == 5


def test_cache_profile_stops_at_the_first_failing_child():
    def script(n, argv, env):
        if n == 1:
            return FakeChild(argv, env, result=None, code=-11)
        return FakeChild(argv, env, answer(argv))

    spawn = Spawner(script)
    out = cotenancy.cache_profile(0, LOW, SIZES, spawn=spawn,
                                  expected_checksum=checksum_of)
    assert out["ok"] is False and out["reason"] == "child-failed"
    assert out["detail"]["returncode"] == -11
    assert len(spawn.log) == 2 and len(out["profile"]) == 1  # nothing after it
    # a wrong checksum is reported, the sweep goes on
    spawn = Spawner(lambda n, argv, env: FakeChild(argv, env, answer(argv, wrong=(n == 0))))
    out = cotenancy.cache_profile(0, LOW, SIZES, spawn=spawn,
                                  expected_checksum=checksum_of)
    assert out["ok"] is False and out["reason"] == "bad-checksum"
    assert len(out["profile"]) == 3
    # too little free memory ends it
    spawn = Spawner(lambda n, argv, env: FakeChild(
        argv, env, {"skipped": "insufficient free memory", "bytes": 1, "free_bytes": 0}))
    out = cotenancy.cache_profile(0, LOW, SIZES, spawn=spawn)
    assert out["reason"] == "insufficient-memory" and len(spawn.log) == 1


# --- agent and CLI ----------------------------------------------------------

def stub_layouts(monkeypatch, layout=LAYOUT, cards=1):
    monkeypatch.setattr(NodeAgent, "mask_layouts",
                        lambda self: {i: dict(layout) for i in range(cards)})


def test_agent_cache_profile_is_gated_like_verify_isolation(monkeypatch):
    spawn = Spawner()
    for layout in ({**LAYOUT, "interleaved": False}, {}, {**LAYOUT, "granule": 7}):
        stub_layouts(monkeypatch, layout)
        assert NodeAgent("n").cache_profile(0, spawn=spawn) == {
            "ok": False, "reason": "unsupported-layout"}
    stub_layouts(monkeypatch)
    assert NodeAgent("n").cache_profile(5, spawn=spawn)["reason"] == "unsupported-layout"
    assert spawn.log == []


def test_agent_cache_profile_runs_the_planner_mask_on_a_scratch_plan(monkeypatch):
    stub_layouts(monkeypatch)
    agent = NodeAgent("n")
    live = agent.mask_plan(0)
    live.allocate("running-tenant", 25)
    spawn = Spawner()
    out = agent.cache_profile(0, spawn=spawn, expected_checksum=checksum_of)
    assert out["ok"] and out["tenant"]["core"] == 50 and out["tenant"]["cus"] == 128
    mask = int(out["tenant"]["mask"], 16)
    assert popcount(mask) == 128 and live.whole_granules(mask)
    assert {c.env[ENV_CU_MASK] for c in spawn.log} == {out["tenant"]["mask"]}
    assert [c.window["bytes"] // MIB for c in spawn.log] == [
        2, 8, 16, 24, 48, 128, 192, 512, 1024]
    assert [e["bytes"] for e in out["profile"]] == [c.window["bytes"] for c in spawn.log]
    spawn = Spawner()
    out = agent.cache_profile(0, share=25, sizes=[MIB], spawn=spawn,
                              expected_checksum=checksum_of)
    assert out["tenant"]["cus"] == 64 and len(spawn.log) == 1
    assert list(agent.mask_plan(0).grants()) == ["running-tenant"]


def test_agent_parser_co_tenancy_cache_flag():
    from elastic_gpu_scheduler_amd.cmd.agent_main import build_parser

    p = build_parser()
    assert p.parse_args(["--co-tenancy"]).co_tenancy_cache is None
    assert p.parse_args(["--co-tenancy", "--co-tenancy-cache"]).co_tenancy_cache == (12, 128)
    assert p.parse_args(["--co-tenancy-cache", "24"]).co_tenancy_cache == (24,)
    assert p.parse_args(["--co-tenancy-cache", "12,128,1024"]).co_tenancy_cache == (
        12, 128, 1024)
    for bad in ("", "0", "12,", "a", "12;128", "1025", "-4"):
        with pytest.raises(SystemExit):
            p.parse_args(["--co-tenancy-cache=" + bad])


def test_agent_main_cache_reports_every_card_and_size_in_turn(monkeypatch, capsys):
    from elastic_gpu_scheduler_amd.cmd import agent_main

    stub_layouts(monkeypatch, cards=2)
    calls = []

    def verify(self, card, shares, **kw):
        calls.append((card, shares, kw))
        return {"ok": True, "n": len(calls)}

    monkeypatch.setattr(NodeAgent, "verify_isolation", verify)
    assert agent_main.main(["--co-tenancy", "25,75", "--co-tenancy-cache", "12,128"]) == 0
    assert [(card, shares) for card, shares, _ in calls] == [
        (0, (25, 75)), (0, (25, 75)), (1, (25, 75)), (1, (25, 75))]
    for (_, _, kw), mib in zip(calls, (12, 128, 12, 128)):
        assert set(kw) == {"pairs", "windows"}
        assert kw["pairs"] == cotenancy.CACHE_PAIRS == (
            ("cache", "cache"), ("cache", "stream"), ("stream", "cache"),
            ("cache", "fma"))
        assert kw["windows"] == {"cache": {
            "bytes": mib << 20, "passes": cotenancy.cache_passes(mib << 20)}}
    assert json.loads(capsys.readouterr().out) == {
        "0": {"12": {"ok": True, "n": 1}, "128": {"ok": True, "n": 2}},
        "1": {"12": {"ok": True, "n": 3}, "128": {"ok": True, "n": 4}}}
    # the cache flag alone measures nothing
    del calls[:]
    assert agent_main.main(["--co-tenancy-cache", "12"]) == 2
    assert calls == [] and capsys.readouterr().out == ""
    with pytest.raises(SystemExit):
        agent_main.main(["--co-tenancy", "--co-tenancy-cache", "12,x"])


# --- binding argument checks ------------------------------------------------

@needs_probe
def test_cache_tenant_rejects_bad_arguments_before_touching_the_device():
    p = gpuprobe()
    for bad in (0, -1, 1 << 300, 1 << 256):
        with pytest.raises(ValueError):
            p.cu_tenant_run(0, kind="cache", mask=bad)
    for kind in ("cach", "Cache", "cache "):
        with pytest.raises(ValueError, match="cache"):
            p.cu_tenant_run(0, kind=kind)
    with pytest.raises(TypeError):
        p.cu_tenant_run(0, kind="cache", mask="0xff")
    assert "cache" in p.cu_tenant_run.__doc__


@needs_probe
def test_cache_tenant_raises_without_device():
    import torch

    if torch.cuda.is_available():
        return  # a device is visible: covered by the gpu-marked tests
    p = gpuprobe()
    with pytest.raises(RuntimeError):
        p.cu_tenant_run(0, kind="cache", launches=1, bytes=16, passes=1)
    with pytest.raises(RuntimeError):
        p.cu_tenant_run(0, mask=0xFF, kind="cache")
