"""The mfma tenant of the interference probe, the parts that need no GPU:
the closed-form oracle against a brute-force model of the kernel (tile by
tile, step by step, chunk by chunk), the exactness of its f32 accumulators,
that the checksum notices what it should, the report's clock split over
(fake) children, and the CLI flag."""
from __future__ import annotations

import json
import subprocess
import threading

import numpy as np
import pytest

from elastic_gpu_scheduler_amd._native import gpuprobe, gpuprobe_available
from elastic_gpu_scheduler_amd.agent import cotenancy
from elastic_gpu_scheduler_amd.agent.agent import NodeAgent
from elastic_gpu_scheduler_amd.agent.cotenancy import isolation_report

needs_probe = pytest.mark.skipif(not gpuprobe_available(),
                                 reason="_gpuprobe extension not built")

LAYOUT = {"cus": 256, "xccs": 8, "granule": 8, "interleaved": True, "lost": []}
LOW, HIGH = (1 << 128) - 1, ((1 << 128) - 1) << 128
TENANTS = [{"mask": LOW}, {"mask": HIGH}]
WORKGROUPS = 8 * 128  # what an mfma child under a 50-share mask of 256 CUs reports
GPU_SEEDS = (0x5EED, 1)  # what tests/test_gpu_mfma_cotenancy.py runs with
CHUNK = 2048


# --- a brute-force model of the kernel ------------------------------------------

def mix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def operands(seed, variant):
    """A (64 x 16) and B (16 x 64) of one variant, as the issue states them."""
    key = mix32((seed & 0xFFFFFFFF) ^ ((variant * 0x9E3779B1) & 0xFFFFFFFF))
    a = np.array([[mix32(key ^ (row << 8) ^ k ^ 0x00A00000) % 31 - 15
                   for k in range(16)] for row in range(64)], dtype=np.int64)
    b = np.array([[mix32(key ^ (k << 8) ^ col ^ 0x00B00000) % 31 - 15
                   for col in range(64)] for k in range(16)], dtype=np.int64)
    return a, b


_PRODUCTS = {}


def product(seed, variant):
    if (seed, variant) not in _PRODUCTS:
        a, b = operands(seed, variant)
        assert np.abs(a).max() <= 15 and np.abs(b).max() <= 15
        _PRODUCTS[seed, variant] = (a @ b).astype(np.float32)
    return _PRODUCTS[seed, variant]


def weights(swap_mn=False):
    """Every element of the 64 x 64 tile is held by exactly one (lane, m, n,
    reg), so the fold weight of an element and the lane that owns it are
    functions of its position. Returns (weight, lane), both 64 x 64."""
    weight = np.zeros((64, 64), dtype=np.int64)
    owner = np.zeros((64, 64), dtype=np.int64)
    seen = np.zeros((64, 64), dtype=bool)
    for lane in range(64):
        r, h = lane & 31, lane >> 5
        for m in range(2):
            for n in range(2):
                for reg in range(16):
                    row = 32 * m + (reg & 3) + 8 * (reg >> 2) + 4 * h
                    col = 32 * n + r
                    assert not seen[row, col]
                    seen[row, col] = True
                    t = 2 * n + m if swap_mn else 2 * m + n
                    weight[row, col] = 1 + reg + 16 * t
                    owner[row, col] = lane
    assert seen.all()
    return weight, owner


def model_checksum(workgroups, iters, seed, *, swap_mn=False, drop_step_in_wave=None,
                   shift_wave=None):
    """Every wave's 64 x 64 tile in f32, one product added per step, zeroed
    at the start of every chunk of 2048 steps and folded per lane at its end
    through the register-to-row map; then every lane weighted by its global
    index. Arithmetic modulo 2^64 throughout, as on the device."""
    weight, owner = weights(swap_mn)
    mask = (1 << 64) - 1
    total = 0
    for w in range(4 * workgroups):
        variant = (w + 1 if w == shift_wave else w) % 16
        p = product(seed, variant)
        steps = iters - 1 if w == drop_step_in_wave else iters
        fold = [0] * 64
        done = 0
        while done < steps:
            n = min(CHUNK, steps - done)
            acc = np.zeros((64, 64), dtype=np.float32)  # explicit reset
            for _ in range(n):
                acc += p
            ints = acc.astype(np.int64)
            assert (ints.astype(np.float32) == acc).all()
            contrib = ints * weight
            for lane in range(64):
                fold[lane] = (fold[lane] + int(contrib[owner == lane].sum())) & mask
            done += n
        for lane in range(64):
            total = (total + (64 * w + lane + 1) * fold[lane]) & mask
    return total


ITERS = (1, 2, 2047, 2048, 2049, 4099)


@pytest.mark.parametrize("workgroups", (1, 3, 5))
def test_mfma_checksum_equals_the_brute_force_model(workgroups):
    """5 workgroups are 20 waves: the 16 variants wrap."""
    for seed in (0x5EED, 0x1_0000_0007):  # the second has bits above the low 32
        for iters in ITERS:
            got = cotenancy.mfma_checksum(workgroups, iters, seed)
            assert 0 <= got < 1 << 64
            assert got == model_checksum(workgroups, iters, seed), (
                workgroups, iters, hex(seed))


def test_mfma_checksum_takes_the_low_32_bits_of_the_seed():
    assert cotenancy.mfma_checksum(2, 3, 0x1_0000_0007) == cotenancy.mfma_checksum(2, 3, 7)
    assert cotenancy.mfma_checksum(2, 3, 7) != cotenancy.mfma_checksum(2, 3, 8)


@pytest.mark.parametrize("seed", GPU_SEEDS)
def test_a_chunk_of_partial_sums_is_exact_in_f32(seed):
    """Integers up to 2^24 are exact in f32: a chunk's largest partial sum
    must stay below that for every variant, at the seeds the GPU tests use."""
    worst = max(float(np.abs(product(seed, v)).max()) for v in range(16))
    print("seed", hex(seed), "max |P| over 16 variants:", worst)
    assert worst <= 16 * 15 * 15
    assert CHUNK * worst < 1 << 24


def test_the_checksum_notices_weights_steps_and_variants():
    seed, iters = 0x5EED, 5
    right = model_checksum(2, iters, seed)
    assert right == cotenancy.mfma_checksum(2, iters, seed)
    assert model_checksum(2, iters, seed, swap_mn=True) != right
    assert model_checksum(2, iters, seed, drop_step_in_wave=3) != right
    assert model_checksum(2, iters, seed, shift_wave=6) != right


# --- kinds, pairs, parser -------------------------------------------------------

def test_mfma_kind_and_pairs_are_added_and_nothing_older_moves():
    assert cotenancy.MATRIX_KINDS == ("mfma",)
    assert cotenancy.ALL_KINDS == cotenancy.KINDS + ("mfma",)
    assert cotenancy.KINDS == ("fma", "stream", "cache", "chase")
    assert cotenancy.MFMA_PAIRS == (("mfma", "mfma"), ("mfma", "stream"),
                                    ("stream", "mfma"), ("mfma", "fma"))


def test_child_parser_accepts_the_mfma_kind():
    args = cotenancy._child_parser().parse_args(
        ["--child", "--kind", "mfma", "--iters", "5"])
    assert (args.kind, args.iters) == ("mfma", 5)
    with pytest.raises(SystemExit):
        cotenancy._child_parser().parse_args(["--child", "--kind", "mfm"])


# --- fake children ------------------------------------------------------------

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
        if self.returncode is None:
            self.returncode = -9
        self._gone.set()
        self._go.set()


SOLO_RATE = {"fma": 100.0, "stream": 40.0, "mfma": 1000.0}
SOLO_CLOCK = 2.0


def checksum_of(seed, nbytes):
    """The fake oracle of the reading kinds: any function of both will do."""
    return (seed * 1_000_003) ^ nbytes


def answer(argv, rate=None, clock=SOLO_CLOCK, wrong=False):
    """What a child given `argv` would print: `launches` back-to-back
    launches of 1000 ticks of a 100 MHz clock, and the checksum of its kind."""
    kind = flag(argv, "--kind")
    count, seed = int(flag(argv, "--launches")), int(flag(argv, "--seed"))
    rate = SOLO_RATE[kind] if rate is None else rate
    out = {"kind": kind, "applied_mask": None, "tick_hz": 1e8,
           "workgroups": WORKGROUPS if kind == "mfma" else 4 * WORKGROUPS,
           "work_per_launch": 1e9, "rate": rate,
           "launches": [{"t0": 100_000 + 1000 * i, "t1": 100_000 + 1000 * i + 999,
                         "seconds": 999 / 1e8, "event_seconds": 1000 / 1e8,
                         "rate": rate} for i in range(count)]}
    if kind == "fma":
        out["iters"] = int(flag(argv, "--iters"))
    elif kind == "mfma":
        iters = int(flag(argv, "--iters")) or 32768
        ticks = 999 * WORKGROUPS
        for l in out["launches"]:
            l.update(cycles=int(clock * 10 * ticks), ticks=ticks, clock_ghz=clock)
        out.update(iters=iters, clock_ghz=clock,
                   checksum=cotenancy.mfma_checksum(WORKGROUPS, iters, seed) ^ wrong)
    else:
        nbytes = int(flag(argv, "--bytes"))
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


NEW_FIELDS = ("solo_clock_ghz", "contended_clock_ghz", "clock_ratio", "cycle_ratio")


# --- isolation_report with the mfma kind ----------------------------------------

def test_report_runs_the_mfma_pairs_and_splits_the_ratio():
    """Solo children 0..4, then the pairs. In every pair the contended mfma
    tenants run at 0.8 of the solo rate and 0.9 of the solo clock."""
    def script(n, argv, env):
        if n >= 5 and flag(argv, "--kind") == "mfma":
            return FakeChild(argv, env, answer(argv, rate=800.0, clock=1.8))
        return FakeChild(argv, env, answer(argv))

    spawn = Spawner(script)
    report = isolation_report(0, TENANTS, pairs=cotenancy.MFMA_PAIRS, launches=8,
                              seed=0x5EED, windows={"mfma": {"iters": 4099}},
                              spawn=spawn, expected_checksum=checksum_of)
    assert report["ok"], report
    assert [c.kind for c in spawn.log] == [
        "stream", "mfma",          # solo, tenant 0: the kinds it has in a pair
        "fma", "stream", "mfma",   # solo, tenant 1
        "mfma", "mfma", "mfma", "stream", "stream", "mfma", "mfma", "fma"]
    assert list(report["pairs"]) == ["mfma/mfma", "mfma/stream", "stream/mfma",
                                     "mfma/fma"]
    for c in spawn.log:
        assert c.window["iters"] == (4099 if c.kind == "mfma" else 0)
        assert c.window["seed"] == 0x5EED
    for i in range(2):
        solo = report["solo"][i]["mfma"]
        assert solo["rate"] == 1000.0 and solo["workgroups"] == WORKGROUPS
        assert solo["clock_ghz"] == SOLO_CLOCK
        assert "clock_ghz" not in report["solo"][i]["stream"]
    assert "clock_ghz" not in report["solo"][1]["fma"]
    for name, pair in report["pairs"].items():
        for t in pair["tenants"]:
            assert t["contended_launches"] == 8
            if t["kind"] != "mfma":
                assert not any(f in t for f in NEW_FIELDS), (name, t)
                assert t["ratio"] == 1.0
                continue
            assert t["solo_clock_ghz"] == 2.0 and t["contended_clock_ghz"] == 1.8
            assert t["ratio"] == pytest.approx(0.8)
            assert t["clock_ratio"] == pytest.approx(0.9)
            assert t["cycle_ratio"] == pytest.approx(0.8 / 0.9)
            assert t["cycle_ratio"] * t["clock_ratio"] == pytest.approx(t["ratio"])
    kinds = [t["kind"] for t in report["pairs"]["mfma/fma"]["tenants"]]
    assert kinds == ["mfma", "fma"]


def test_report_wrong_mfma_checksum_is_not_ok():
    def script(n, argv, env):  # three solo runs, then child 4: second of mfma/mfma
        return FakeChild(argv, env, answer(argv, wrong=(n == 4)))

    report = isolation_report(0, TENANTS, pairs=[("mfma", "mfma"), ("mfma", "fma")],
                              spawn=Spawner(script), expected_checksum=checksum_of)
    assert not report["ok"] and report["reason"] == "bad-checksum"
    pair = report["pairs"]["mfma/mfma"]
    assert not pair["ok"] and pair["tenants"][1]["reason"] == "bad-checksum"
    assert "reason" not in pair["tenants"][0]
    assert report["pairs"]["mfma/fma"]["ok"]
    # a solo mfma run's checksum counts too
    spawn = Spawner(lambda n, argv, env: FakeChild(argv, env, answer(argv, wrong=(n == 0))))
    report = isolation_report(0, TENANTS, pairs=[("mfma", "mfma")], spawn=spawn)
    assert not report["ok"] and report["reason"] == "bad-checksum"


def test_report_with_too_little_overlap_has_no_clock_split():
    def script(n, argv, env):  # child 3 runs long after child 2
        out = answer(argv)
        if n == 3:
            for l in out["launches"]:
                l["t0"] += 10 ** 9
                l["t1"] += 10 ** 9
        return FakeChild(argv, env, out)

    report = isolation_report(0, TENANTS, pairs=[("mfma", "mfma")], spawn=Spawner(script))
    assert not report["ok"] and report["reason"] == "no-overlap"
    for t in report["pairs"]["mfma/mfma"]["tenants"]:
        assert "ratio" not in t and not any(f in t for f in NEW_FIELDS)


def test_report_takes_an_mfma_window_and_refuses_unknown_kinds_before_spawning():
    spawn = Spawner()
    for pairs in ([("mfma", "mfm")], [("matrix", "stream")], [("mfma",)]):
        with pytest.raises(ValueError):
            isolation_report(0, TENANTS, pairs=pairs, spawn=spawn)
    with pytest.raises(ValueError):
        isolation_report(0, TENANTS, pairs=cotenancy.MFMA_PAIRS,
                         windows={"mfma": {"steps": 16}}, spawn=spawn)
    with pytest.raises(ValueError, match="unknown tenant kind"):
        cotenancy.run_pair(0, [{"mask": LOW, "kind": "mfm"}], spawn=spawn)
    assert spawn.log == []


# --- agent and CLI --------------------------------------------------------------

def stub_layouts(monkeypatch, layout=LAYOUT, cards=1):
    monkeypatch.setattr(NodeAgent, "mask_layouts",
                        lambda self: {i: dict(layout) for i in range(cards)})


def test_agent_parser_co_tenancy_mfma_flag():
    from elastic_gpu_scheduler_amd.cmd.agent_main import build_parser

    p = build_parser()
    assert p.parse_args(["--co-tenancy"]).co_tenancy_mfma is False
    args = p.parse_args(["--co-tenancy", "--co-tenancy-mfma"])
    assert args.co_tenancy_mfma is True and args.co_tenancy == (50, 50)
    assert args.co_tenancy_cache is None and args.co_tenancy_chase is None
    with pytest.raises(SystemExit):  # a plain flag: it takes no value
        p.parse_args(["--co-tenancy-mfma=12"])


def test_agent_main_mfma_reports_every_card_in_turn(monkeypatch, capsys):
    from elastic_gpu_scheduler_amd.cmd import agent_main

    stub_layouts(monkeypatch, cards=2)
    calls = []

    def verify(self, card, shares, **kw):
        calls.append((card, shares, kw))
        return {"ok": True, "n": len(calls)}

    monkeypatch.setattr(NodeAgent, "verify_isolation", verify)
    assert agent_main.main(["--co-tenancy", "25,75", "--co-tenancy-mfma"]) == 0
    assert calls == [(0, (25, 75), {"pairs": cotenancy.MFMA_PAIRS}),
                     (1, (25, 75), {"pairs": cotenancy.MFMA_PAIRS})]
    assert json.loads(capsys.readouterr().out) == {
        "0": {"ok": True, "n": 1}, "1": {"ok": True, "n": 2}}
    # the flag alone, or beside either of the other two, measures nothing
    del calls[:]
    assert agent_main.main(["--co-tenancy-mfma"]) == 2
    out, err = capsys.readouterr()
    assert calls == [] and out == "" and "--co-tenancy" in err
    for other in (["--co-tenancy-chase", "2"], ["--co-tenancy-cache", "12"]):
        assert agent_main.main(["--co-tenancy", "--co-tenancy-mfma"] + other) == 2
        out, err = capsys.readouterr()
        assert calls == [] and out == "" and other[0] in err


def test_agent_verify_isolation_passes_the_mfma_pairs_through(monkeypatch):
    stub_layouts(monkeypatch)
    spawn = Spawner()
    report = NodeAgent("n").verify_isolation(0, (50, 50), pairs=cotenancy.MFMA_PAIRS,
                                             spawn=spawn, expected_checksum=checksum_of)
    assert report["ok"], report
    assert list(report["pairs"]) == ["mfma/mfma", "mfma/stream", "stream/mfma", "mfma/fma"]
    assert [t["cus"] for t in report["tenants"]] == [128, 128]
    assert "MFMA_PAIRS" in NodeAgent.verify_isolation.__doc__


# --- binding argument checks ------------------------------------------------

@needs_probe
def test_mfma_tenant_rejects_bad_arguments_before_touching_the_device():
    p = gpuprobe()
    for bad in (0, -1, 1 << 300, 1 << 256):
        with pytest.raises(ValueError):
            p.cu_tenant_run(0, kind="mfma", mask=bad)
    for kind in ("mfm", "MFMA", "mfma "):
        with pytest.raises(ValueError, match="mfma"):
            p.cu_tenant_run(0, kind=kind)
    with pytest.raises(TypeError):
        p.cu_tenant_run(0, kind="mfma", mask="0xff")
    doc = p.cu_tenant_run.__doc__
    assert "mfma" in doc and "clock_ghz" in doc and "small integers" in doc
    assert "real GEMM" in doc


@needs_probe
def test_mfma_tenant_raises_without_device():
    import torch

    if torch.cuda.is_available():
        return  # a device is visible: covered by the gpu-marked tests
    p = gpuprobe()
    with pytest.raises(RuntimeError):  # ValueError while the kind is unknown
        p.cu_tenant_run(0, kind="mfma", launches=1, iters=1)
    with pytest.raises(RuntimeError):
        p.cu_tenant_run(0, mask=0xFF, kind="mfma")
