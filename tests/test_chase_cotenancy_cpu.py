"""The chase tenant of the interference probe, the parts that need no GPU:
the closed-form oracle against a brute-force walk, the report's checksum
check for the new kind, the latency sweep over (fake) children, the agent's
gate, the CLI flag, and the probe's argument checks."""
from __future__ import annotations

import json
import math
import subprocess
import threading

import pytest

from elastic_gpu_scheduler_amd._native import gpuprobe, gpuprobe_available
from elastic_gpu_scheduler_amd.agent import cotenancy
from elastic_gpu_scheduler_amd.agent.agent import NodeAgent
from elastic_gpu_scheduler_amd.agent.cotenancy import isolation_report
from elastic_gpu_scheduler_amd.agent.cumask import mask_hex, popcount
from elastic_gpu_scheduler_amd.agent.wiring import ENV_CU_MASK

needs_probe = pytest.mark.skipif(not gpuprobe_available(),
                                 reason="_gpuprobe extension not built")

LAYOUT = {"cus": 256, "xccs": 8, "granule": 8, "interleaved": True, "lost": []}
LOW, HIGH = (1 << 128) - 1, ((1 << 128) - 1) << 128
MIB = 1 << 20
CHASE_BYTES, CHASE_ITERS = 64 * MIB, 4099
WINDOWS = {"chase": {"bytes": CHASE_BYTES, "iters": CHASE_ITERS}}
SOLO_RATE = {"fma": 100.0, "stream": 40.0, "chase": 2.0}
WORKGROUPS = 128  # what a child under a 50-share mask of 256 CUs reports


def checksum_of(seed, nbytes):
    """The fake oracle of the reading kinds: any function of both will do."""
    return (seed * 1_000_003) ^ nbytes


# --- the oracle ---------------------------------------------------------------

NODES = (1, 2, 3, 77, 1021, 4097)


@pytest.mark.parametrize("nodes", NODES + (4, 5, 16, 1024, 16384, 1 << 23, 1 << 27))
def test_chase_stride_is_coprime_and_inside_the_buffer(nodes):
    stride = cotenancy.chase_stride(nodes)
    if nodes == 1:
        assert stride == 0
    else:
        assert 1 <= stride < nodes
        assert stride >= nodes * 28657 // 46368
    assert math.gcd(stride, nodes) == 1


@pytest.mark.parametrize("nodes", NODES)
def test_chase_chain_is_one_cycle_through_every_node(nodes):
    stride = cotenancy.chase_stride(nodes)
    at, hops = stride % nodes, 1
    while at != 0:
        at, hops = (at + stride) % nodes, hops + 1
    assert hops == nodes


def brute_checksum(nodes, workgroups, iters, seed):
    """The buffer laid out as a list, walked hop by hop; then every lane."""
    stride = cotenancy.chase_stride(nodes)
    nxt = [(i + stride) % nodes for i in range(nodes)]
    waves = 4 * workgroups
    total = 0
    for w in range(waves):
        at = (seed + w * nodes // waves) % nodes
        for _ in range(iters):
            at = nxt[at]
        for lane in range(64):
            g = 64 * w + lane
            total += (g + 1) * (at + 1)
    return total % (1 << 64)


@pytest.mark.parametrize("nodes", NODES)
def test_chase_checksum_equals_a_brute_force_walk(nodes):
    for iters in (1, 2, 5, 4099):
        for seed in (0, 1, 0x5EED):
            assert cotenancy.chase_checksum(128 * nodes, 8, iters, seed) == \
                brute_checksum(nodes, 8, iters, seed), (nodes, iters, seed)


def test_chase_checksum_stays_below_two_to_the_64():
    # 1024 waves whose end nodes are near 2^27: the plain sum is far above 2^64
    nbytes = 16 << 30
    plain = sum((64 * 64 * w + 2080) * (
        (w * (nbytes // 128) // 1024 + 4194304 * cotenancy.chase_stride(nbytes // 128))
        % (nbytes // 128) + 1) for w in range(1024))
    got = cotenancy.chase_checksum(nbytes, 256, 4194304, 0)
    assert got == plain % (1 << 64) and 0 <= got < 1 << 64


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
    launches of 1000 ticks from `start`, the window it was asked for and the
    checksum of its kind: the pattern's stand-in for a streamer, the closed
    form for a chase tenant."""
    kind = flag(argv, "--kind")
    count, nbytes = int(flag(argv, "--launches")), int(flag(argv, "--bytes"))
    seed = int(flag(argv, "--seed"))
    rate = SOLO_RATE[kind] if rate is None else rate
    out = {"kind": kind, "applied_mask": None, "tick_hz": 1e8,
           "workgroups": WORKGROUPS if kind == "chase" else 32 * WORKGROUPS,
           "work_per_launch": 1e9, "rate": rate,
           "launches": [{"t0": start + 1000 * i, "t1": start + 1000 * i + 999,
                         "seconds": 999 / 1e8, "event_seconds": 1000 / 1e8,
                         "rate": rate} for i in range(count)]}
    if kind == "fma":
        out["iters"] = int(flag(argv, "--iters"))
    elif kind == "chase":
        nbytes = (nbytes or 1 << 30) // 128 * 128
        iters = int(flag(argv, "--iters")) or 65536
        out.update(bytes=nbytes, nodes=nbytes // 128,
                   stride=cotenancy.chase_stride(nbytes // 128), iters=iters,
                   ns_per_hop=999 / 1e8 * 1e9 / iters,
                   checksum=cotenancy.chase_checksum(nbytes, WORKGROUPS, iters, seed)
                   ^ wrong)
    else:
        out.update(bytes=nbytes, passes=int(flag(argv, "--passes")) | 1,
                   checksum=checksum_of(seed, nbytes) ^ wrong)
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


# --- kinds and pairs ----------------------------------------------------------

def test_child_parser_accepts_the_chase_kind():
    args = cotenancy._child_parser().parse_args(
        ["--child", "--kind", "chase", "--bytes", "4096", "--iters", "5"])
    assert (args.kind, args.bytes, args.iters) == ("chase", 4096, 5)
    assert "chase" in cotenancy.KINDS
    with pytest.raises(SystemExit):
        cotenancy._child_parser().parse_args(["--child", "--kind", "chas"])


def test_chase_pairs_are_added_and_nothing_older_moves():
    assert cotenancy.CHASE_PAIRS == (("chase", "chase"), ("chase", "stream"),
                                     ("stream", "chase"), ("chase", "fma"))
    assert cotenancy.KINDS[:3] == ("fma", "stream", "cache")
    assert cotenancy.KINDS == ("fma", "stream", "cache", "chase")
    assert cotenancy.ALL_PAIRS == (("fma", "fma"), ("stream", "stream"),
                                   ("fma", "stream"), ("stream", "fma"))
    assert cotenancy.CACHE_PAIRS == (("cache", "cache"), ("cache", "stream"),
                                     ("stream", "cache"), ("cache", "fma"))
    assert cotenancy.READING_KINDS == ("stream", "cache")
    assert cotenancy.WINDOW_KEYS == ("iters", "bytes", "passes")


# --- isolation_report with the chase kind -------------------------------------

def test_report_runs_the_chase_pairs_with_the_window_solo_and_paired():
    spawn = Spawner()
    asked = []

    def expected(seed, nbytes):
        asked.append(nbytes)
        return checksum_of(seed, nbytes)

    report = isolation_report(0, TENANTS, pairs=cotenancy.CHASE_PAIRS, launches=8,
                              iters=32, seed=3, windows=WINDOWS, spawn=spawn,
                              expected_checksum=expected)
    assert report["ok"], report
    assert [c.kind for c in spawn.log] == [
        "stream", "chase",          # solo, tenant 0: the kinds it has in a pair
        "fma", "stream", "chase",   # solo, tenant 1
        "chase", "chase", "chase", "stream", "stream", "chase", "chase", "fma"]
    assert list(report["pairs"]) == ["chase/chase", "chase/stream", "stream/chase",
                                     "chase/fma"]
    for c in spawn.log:
        want = {"launches": 8, "iters": 32, "bytes": 0, "passes": 0, "seed": 3}
        want.update(WINDOWS.get(c.kind, {}))
        assert c.window == want, (c.kind, c.window)
    assert spawn.log[1].argv[1:] == [
        "-m", "elastic_gpu_scheduler_amd.agent.cotenancy", "--child",
        "--device", "0", "--kind", "chase", "--launches", "8",
        "--iters", str(CHASE_ITERS), "--bytes", str(CHASE_BYTES), "--passes", "0",
        "--seed", "3"]
    assert [c.env[ENV_CU_MASK] for c in spawn.log[5:]] == [mask_hex(LOW),
                                                           mask_hex(HIGH)] * 4
    assert asked == [0]  # the pattern's oracle serves the streamer alone
    for i in range(2):
        solo = report["solo"][i]["chase"]
        assert solo["rate"] == 2.0 and solo["workgroups"] == WORKGROUPS
        assert solo["ns_per_hop"] == pytest.approx(999 / 1e8 * 1e9 / CHASE_ITERS)
        assert "ns_per_hop" not in report["solo"][i]["stream"]
    assert "ns_per_hop" not in report["solo"][1]["fma"]
    for pair in report["pairs"].values():
        for t in pair["tenants"]:
            assert t["contended_launches"] == 8 and t["ratio"] == 1.0


def test_report_wrong_chase_checksum_is_not_ok():
    def script(n, argv, env):  # three solo runs, then child 4: second of chase/chase
        return FakeChild(argv, env, answer(argv, wrong=(n == 4)))

    report = isolation_report(0, TENANTS, pairs=[("chase", "chase"), ("chase", "fma")],
                              windows=WINDOWS, spawn=Spawner(script),
                              expected_checksum=checksum_of)
    assert not report["ok"] and report["reason"] == "bad-checksum"
    pair = report["pairs"]["chase/chase"]
    assert not pair["ok"] and pair["tenants"][1]["reason"] == "bad-checksum"
    assert "reason" not in pair["tenants"][0]
    assert report["pairs"]["chase/fma"]["ok"]
    # a solo chase run's checksum counts too
    spawn = Spawner(lambda n, argv, env: FakeChild(argv, env, answer(argv, wrong=(n == 0))))
    report = isolation_report(0, TENANTS, pairs=[("chase", "chase")], windows=WINDOWS,
                              spawn=spawn, expected_checksum=checksum_of)
    assert not report["ok"] and report["reason"] == "bad-checksum"
    # and it is the call's seed that the closed form is given
    spawn = Spawner()
    assert isolation_report(0, TENANTS, pairs=[("chase", "chase")], windows=WINDOWS,
                            seed=0x5EED, spawn=spawn)["ok"]


def test_report_still_refuses_unknown_kinds_before_spawning():
    spawn = Spawner()
    for pairs in ([("chase", "chas")], [("pointer", "stream")], [("chase",)]):
        with pytest.raises(ValueError):
            isolation_report(0, TENANTS, pairs=pairs, spawn=spawn)
    with pytest.raises(ValueError):
        isolation_report(0, TENANTS, pairs=cotenancy.CHASE_PAIRS,
                         windows={"chas": {"bytes": 128}}, spawn=spawn)
    with pytest.raises(ValueError):
        isolation_report(0, TENANTS, pairs=cotenancy.CHASE_PAIRS,
                         windows={"chase": {"hops": 16}}, spawn=spawn)
    assert spawn.log == []


# --- chase_profile ----------------------------------------------------------

SIZES = [2 * MIB, 64 * MIB, 1024 * MIB]


def test_chase_profile_one_child_per_size_in_order():
    spawn = Spawner(lambda n, argv, env: FakeChild(
        argv, env, answer(argv, rate=3.0 / (n + 1))))
    out = cotenancy.chase_profile(1, LOW, SIZES, launches=4, seed=7, spawn=spawn)
    assert out["ok"] and len(spawn.log) == 3
    assert [c.kind for c in spawn.log] == ["chase"] * 3
    assert [c.window["bytes"] for c in spawn.log] == SIZES
    assert all(c.window == {"launches": 4, "iters": 0, "bytes": c.window["bytes"],
                            "passes": 0, "seed": 7} for c in spawn.log)
    assert all(c.env[ENV_CU_MASK] == mask_hex(LOW) for c in spawn.log)
    assert all(flag(c.argv, "--device") == "1" for c in spawn.log)
    assert out["profile"] == [
        {"bytes": size, "nodes": size // 128, "iters": 65536,
         "ns_per_hop": pytest.approx(999 / 1e8 * 1e9 / 65536),
         "rate": 3.0 / (n + 1), "seconds": 999 / 1e8}
        for n, size in enumerate(SIZES)]
    # given iters are passed on
    spawn = Spawner()
    out = cotenancy.chase_profile(0, LOW, SIZES[:1], iters=5, spawn=spawn)
    assert spawn.log[0].window["iters"] == 5 and out["profile"][0]["iters"] == 5


def test_chase_profile_stops_at_the_first_failing_child():
    def script(n, argv, env):
        if n == 1:
            return FakeChild(argv, env, result=None, code=-11)
        return FakeChild(argv, env, answer(argv))

    spawn = Spawner(script)
    out = cotenancy.chase_profile(0, LOW, SIZES, spawn=spawn)
    assert out["ok"] is False and out["reason"] == "child-failed"
    assert out["detail"]["returncode"] == -11
    assert len(spawn.log) == 2 and len(out["profile"]) == 1  # nothing after it
    # a wrong checksum is reported, the sweep goes on
    spawn = Spawner(lambda n, argv, env: FakeChild(argv, env, answer(argv, wrong=(n == 0))))
    out = cotenancy.chase_profile(0, LOW, SIZES, spawn=spawn)
    assert out["ok"] is False and out["reason"] == "bad-checksum"
    assert len(out["profile"]) == 3
    # too little free memory ends it
    spawn = Spawner(lambda n, argv, env: FakeChild(
        argv, env, {"skipped": "insufficient free memory", "bytes": 1, "free_bytes": 0}))
    out = cotenancy.chase_profile(0, LOW, SIZES, spawn=spawn)
    assert out["ok"] is False and out["reason"] == "insufficient-memory"
    assert len(spawn.log) == 1 and out["profile"] == []


# --- agent and CLI ----------------------------------------------------------

def stub_layouts(monkeypatch, layout=LAYOUT, cards=1):
    monkeypatch.setattr(NodeAgent, "mask_layouts",
                        lambda self: {i: dict(layout) for i in range(cards)})


def test_agent_chase_profile_is_gated_like_cache_profile(monkeypatch):
    spawn = Spawner()
    for layout in ({**LAYOUT, "interleaved": False}, {}, {**LAYOUT, "granule": 7}):
        stub_layouts(monkeypatch, layout)
        assert NodeAgent("n").chase_profile(0, spawn=spawn) == {
            "ok": False, "reason": "unsupported-layout"}
    stub_layouts(monkeypatch)
    assert NodeAgent("n").chase_profile(5, spawn=spawn)["reason"] == "unsupported-layout"
    assert spawn.log == []


def test_agent_chase_profile_runs_the_planner_mask_on_a_scratch_plan(monkeypatch):
    stub_layouts(monkeypatch)
    agent = NodeAgent("n")
    live = agent.mask_plan(0)
    live.allocate("running-tenant", 25)
    spawn = Spawner()
    out = agent.chase_profile(0, spawn=spawn)
    assert out["ok"] and out["tenant"]["core"] == 50 and out["tenant"]["cus"] == 128
    mask = int(out["tenant"]["mask"], 16)
    assert popcount(mask) == 128 and live.whole_granules(mask)
    assert {c.env[ENV_CU_MASK] for c in spawn.log} == {out["tenant"]["mask"]}
    assert [c.window["bytes"] // MIB for c in spawn.log] == [
        1, 2, 4, 8, 32, 64, 128, 256, 512, 1024]
    assert [e["bytes"] for e in out["profile"]] == [c.window["bytes"] for c in spawn.log]
    spawn = Spawner()
    out = agent.chase_profile(0, share=25, sizes=[MIB], iters=9, spawn=spawn)
    assert out["tenant"]["cus"] == 64 and len(spawn.log) == 1
    assert spawn.log[0].window["iters"] == 9
    assert list(agent.mask_plan(0).grants()) == ["running-tenant"]


def test_agent_parser_co_tenancy_chase_flag():
    from elastic_gpu_scheduler_amd.cmd.agent_main import build_parser

    p = build_parser()
    assert p.parse_args(["--co-tenancy"]).co_tenancy_chase is None
    assert p.parse_args(["--co-tenancy", "--co-tenancy-chase"]).co_tenancy_chase == (
        2, 64, 1024)
    assert p.parse_args(["--co-tenancy-chase", "24"]).co_tenancy_chase == (24,)
    assert p.parse_args(["--co-tenancy-chase", "2,64"]).co_tenancy_chase == (2, 64)
    assert p.parse_args(["--co-tenancy", "--co-tenancy-chase"]).co_tenancy_cache is None
    for bad in ("", "0", "12,", "a", "12;128", "1025", "-4"):
        with pytest.raises(SystemExit):
            p.parse_args(["--co-tenancy-chase=" + bad])


def test_agent_main_chase_reports_every_card_and_size_in_turn(monkeypatch, capsys):
    from elastic_gpu_scheduler_amd.cmd import agent_main

    stub_layouts(monkeypatch, cards=2)
    calls = []

    def verify(self, card, shares, **kw):
        calls.append((card, shares, kw))
        return {"ok": True, "n": len(calls)}

    monkeypatch.setattr(NodeAgent, "verify_isolation", verify)
    assert agent_main.main(["--co-tenancy", "25,75", "--co-tenancy-chase", "2,64"]) == 0
    assert [(card, shares) for card, shares, _ in calls] == [
        (0, (25, 75)), (0, (25, 75)), (1, (25, 75)), (1, (25, 75))]
    for (_, _, kw), mib in zip(calls, (2, 64, 2, 64)):
        assert set(kw) == {"pairs", "windows"}
        assert kw["pairs"] == cotenancy.CHASE_PAIRS
        assert kw["windows"] == {"chase": {"bytes": mib << 20}}
    assert json.loads(capsys.readouterr().out) == {
        "0": {"2": {"ok": True, "n": 1}, "64": {"ok": True, "n": 2}},
        "1": {"2": {"ok": True, "n": 3}, "64": {"ok": True, "n": 4}}}
    # the chase flag alone, or beside the cache flag, measures nothing
    del calls[:]
    assert agent_main.main(["--co-tenancy-chase", "2"]) == 2
    out, err = capsys.readouterr()
    assert calls == [] and out == "" and "--co-tenancy" in err
    assert agent_main.main(["--co-tenancy", "--co-tenancy-chase", "2",
                            "--co-tenancy-cache", "12"]) == 2
    out, err = capsys.readouterr()
    assert calls == [] and out == "" and "--co-tenancy-cache" in err
    with pytest.raises(SystemExit):
        agent_main.main(["--co-tenancy", "--co-tenancy-chase", "2,x"])


def test_verify_isolation_docstring_names_the_chase_pairs():
    assert "CHASE_PAIRS" in NodeAgent.verify_isolation.__doc__


# --- binding argument checks ------------------------------------------------

@needs_probe
def test_chase_tenant_rejects_bad_arguments_before_touching_the_device():
    p = gpuprobe()
    for bad in (0, -1, 1 << 300, 1 << 256):
        with pytest.raises(ValueError):
            p.cu_tenant_run(0, kind="chase", mask=bad)
    for kind in ("chas", "Chase", "chase "):
        with pytest.raises(ValueError, match="chase"):
            p.cu_tenant_run(0, kind=kind)
    with pytest.raises(TypeError):
        p.cu_tenant_run(0, kind="chase", mask="0xff")
    doc = p.cu_tenant_run.__doc__
    assert "chase" in doc and "ns_per_hop" in doc and "4 MiB" in doc


@needs_probe
def test_chase_tenant_raises_without_device():
    import torch

    if torch.cuda.is_available():
        return  # a device is visible: covered by the gpu-marked tests
    p = gpuprobe()
    with pytest.raises(RuntimeError):  # ValueError while the kind is unknown
        p.cu_tenant_run(0, kind="chase", launches=1, bytes=128, iters=1)
    with pytest.raises(RuntimeError):
        p.cu_tenant_run(0, mask=0xFF, kind="chase")
