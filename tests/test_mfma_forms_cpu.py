"""The forms of the mfma tenant (bf16, fp8, mxfp8, mxfp4), the parts that need
no GPU: the closed-form oracle of every form against a brute-force model of
the kernel written from the forms' rules alone (numpy matrices, f32
accumulation step by step, zeroed and folded at the form's chunk), the
bounds that make a chunk exact, that the model notices what it should, the
form on its way through run_pair, isolation_report and the CLI over (fake)
children, and the binding's argument checks."""
from __future__ import annotations

import json
import subprocess
import threading

import numpy as np
import pytest

from elastic_gpu_scheduler_amd._native import gpuprobe, gpuprobe_available
from elastic_gpu_scheduler_amd.agent import cotenancy
from elastic_gpu_scheduler_amd.agent.agent import NodeAgent
from elastic_gpu_scheduler_amd.agent.cotenancy import isolation_report, run_pair

needs_probe = pytest.mark.skipif(not gpuprobe_available(),
                                 reason="_gpuprobe extension not built")

LAYOUT = {"cus": 256, "xccs": 8, "granule": 8, "interleaved": True, "lost": []}
LOW, HIGH = (1 << 128) - 1, ((1 << 128) - 1) << 128
TENANTS = [{"mask": LOW}, {"mask": HIGH}]
WORKGROUPS = 8 * 128  # what an mfma child under a 50-share mask of 256 CUs reports
GPU_SEEDS = (0x5EED, 1)  # what tests/test_gpu_mfma_forms.py runs with

FORMS = ("bf16", "fp8", "mxfp8", "mxfp4")
NEW_FORMS = FORMS[1:]
SCALED_FORMS = ("mxfp8", "mxfp4")
# form: (id, K, flop per MFMA, chunk, default iters, max |A|, max |B|)
RULES = {
    "bf16": (0, 16, 32768, 2048, 32768, 15, 15),
    "fp8": (1, 16, 32768, 2048, 32768, 15, 15),
    "mxfp8": (2, 64, 131072, 512, 16384, 14, 14),
    "mxfp4": (3, 64, 131072, 256, 32768, 24, 12),
}
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


# --- a brute-force model of the kernel ------------------------------------------

def mix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def operands(form, seed, variant, flip=None):
    """Effective A (64 x K) and B (K x 64) of one variant, in float64: the
    stored element times 2^(scale byte - 127) of its block of 32 k. `flip`
    = (row, blk) flips that one scale bit of A."""
    f, depth = RULES[form][0], RULES[form][1]
    key = mix32((seed & 0xFFFFFFFF) ^ ((variant * 0x9E3779B1) & 0xFFFFFFFF))
    a = np.zeros((64, depth))
    b = np.zeros((depth, 64))
    for x in range(64):
        for k in range(depth):
            ha = mix32(key ^ (x << 8) ^ k ^ 0x00A00000 ^ (f << 24))
            hb = mix32(key ^ (k << 8) ^ x ^ 0x00B00000 ^ (f << 24))
            blk = k // 32
            ea = mix32(key ^ (x << 8) ^ blk ^ 0x00E00000 ^ (f << 24)) & 1
            eb = mix32(key ^ (blk << 8) ^ x ^ 0x00F00000 ^ (f << 24)) & 1
            if flip == (x, blk):
                ea ^= 1
            if form in ("bf16", "fp8"):
                va, vb = ha % 31 - 15, hb % 31 - 15
            elif form == "mxfp8":
                va = (ha % 15 - 7) * 2.0 ** ((127 + ea) - 127)
                vb = (hb % 15 - 7) * 2.0 ** ((127 + eb) - 127)
            else:
                ca, cb = ha & 15, hb & 15
                va = (-1 if ca & 8 else 1) * E2M1[ca & 7] * 2.0 ** ((128 + ea) - 127)
                vb = (-1 if cb & 8 else 1) * E2M1[cb & 7] * 2.0 ** (128 - 127)
            a[x, k], b[k, x] = va, vb
    return a, b


_PRODUCTS = {}


def product(form, seed, variant, flip=None):
    key = (form, seed & 0xFFFFFFFF, variant, flip)
    if key not in _PRODUCTS:
        a, b = operands(form, seed, variant, flip)
        assert (a == np.round(a)).all() and (b == np.round(b)).all()
        assert np.abs(a).max() <= RULES[form][5] and np.abs(b).max() <= RULES[form][6]
        _PRODUCTS[key] = (a @ b).astype(np.float32)
    return _PRODUCTS[key]


def weights(swap_mn=False):
    """Every element of the 64 x 64 tile is held by exactly one (lane, m, n,
    reg): lane r + 32 h holds in register reg of accumulator (m, n) row 32 m
    + (reg & 3) + 8 (reg >> 2) + 4 h of column 32 n + r, for every form.
    Returns (weight, lane), both 64 x 64."""
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


_WEIGHTS = {False: weights(False), True: weights(True)}
_FOLDS = {}


def wave_folds(form, seed, variant, steps, swap_mn=False, flip=None):
    """The 64 lanes' folds of one wave: its tile in f32, one product added
    per step, zeroed at the start of every chunk and folded at its end."""
    key = (form, seed & 0xFFFFFFFF, variant, steps, swap_mn, flip)
    if key in _FOLDS:
        return _FOLDS[key]
    weight, owner = _WEIGHTS[swap_mn]
    chunk = RULES[form][3]
    p = product(form, seed, variant, flip)
    mask = (1 << 64) - 1
    fold = [0] * 64
    done = 0
    while done < steps:
        n = min(chunk, steps - done)
        acc = np.zeros((64, 64), dtype=np.float32)  # explicit reset
        for _ in range(n):
            acc += p
        ints = acc.astype(np.int64)
        assert (ints.astype(np.float32) == acc).all()
        assert (ints == p.astype(np.int64) * n).all()  # integer-exact
        contrib = ints * weight
        for lane in range(64):
            fold[lane] = (fold[lane] + int(contrib[owner == lane].sum())) & mask
        done += n
    _FOLDS[key] = fold
    return fold


def model_checksum(form, workgroups, iters, seed, *, swap_mn=False,
                   drop_step_in_wave=None, shift_wave=None, flip=None):
    """Every lane weighted by its global index, modulo 2^64 as on the device."""
    mask = (1 << 64) - 1
    total = 0
    for w in range(4 * workgroups):
        variant = (w + 1 if w == shift_wave else w) % 16
        steps = iters - 1 if w == drop_step_in_wave else iters
        fold = wave_folds(form, seed, variant, steps, swap_mn,
                          flip if variant == 0 else None)
        for lane in range(64):
            total = (total + (64 * w + lane + 1) * fold[lane]) & mask
    return total


def iters_around(form):
    chunk = RULES[form][3]
    return (1, 2, chunk - 1, chunk, chunk + 1, 2 * chunk + 3)


@pytest.mark.parametrize("workgroups", (1, 3, 5))
@pytest.mark.parametrize("form", FORMS)
def test_mfma_checksum_of_a_form_equals_the_brute_force_model(form, workgroups):
    """5 workgroups are 20 waves: the 16 variants wrap."""
    for seed in (0x5EED, 0x1_0000_0007):  # the second has bits above the low 32
        for iters in iters_around(form):
            got = cotenancy.mfma_checksum(workgroups, iters, seed, form=form)
            assert 0 <= got < 1 << 64
            assert got == model_checksum(form, workgroups, iters, seed), (
                form, workgroups, iters, hex(seed))


def test_the_issue_s_cross_check_values():
    """From a CPU prototype of the rules, independent of module and model."""
    small = {"bf16": 1473222840, "fp8": 2264415480, "mxfp8": 1817877846,
             "mxfp4": 4158640977}
    large = {"fp8": 18409058969200509184, "mxfp8": 111092423174254080,
             "mxfp4": 243348556056705024}
    for form, want in small.items():
        assert cotenancy.mfma_checksum(2, 3, 0x5EED, form) == want, form
        assert model_checksum(form, 2, 3, 0x5EED) == want, form
    for form, want in large.items():
        assert cotenancy.mfma_checksum(1024, 2049, 1, form=form) == want, form


def test_bf16_is_the_default_and_is_unchanged():
    for args in ((2, 3, 0x5EED), (1024, 2049, 1), (5, 4099, 0x1_0000_0007)):
        assert cotenancy.mfma_checksum(*args, form="bf16") == cotenancy.mfma_checksum(*args)
        assert cotenancy.mfma_checksum(*args, "bf16") == cotenancy.mfma_checksum(*args)
    assert cotenancy.mfma_checksum(2, 3, 0x5EED) == 1473222840


def test_the_four_forms_give_four_checksums():
    for args in ((2, 3, 0x5EED), (1024, 2049, 1)):
        assert len({cotenancy.mfma_checksum(*args, form=f) for f in FORMS}) == 4


def test_forms_and_their_table():
    assert cotenancy.MFMA_FORMS == FORMS
    assert set(cotenancy.MFMA_FORM_TABLE) == set(FORMS)
    for form, (_, depth, flop, chunk, iters, _, _) in RULES.items():
        assert cotenancy.MFMA_FORM_TABLE[form] == {
            "k": depth, "flop": flop, "chunk": chunk, "iters": iters}
        assert flop == 2 * 32 * 32 * depth
    for bad in ("fp4", "BF16", "", None, 1):
        with pytest.raises(ValueError, match="mxfp4"):
            cotenancy.mfma_checksum(2, 3, 1, form=bad)
    # nothing older moves
    assert cotenancy.KINDS == ("fma", "stream", "cache", "chase")
    assert cotenancy.MATRIX_KINDS == ("mfma",)
    assert cotenancy.WINDOW_KEYS == ("iters", "bytes", "passes")


@pytest.mark.parametrize("form", NEW_FORMS)
def test_a_chunk_of_partial_sums_is_exact_in_f32(form):
    """The derived bound: K * max |A| * max |B| per step, times the chunk,
    below 2^23; and the operands at the seeds the GPU tests use keep to it."""
    _, depth, _, chunk, _, max_a, max_b = RULES[form]
    bound = depth * max_a * max_b
    assert bound == {"fp8": 3600, "mxfp8": 12544, "mxfp4": 18432}[form]
    assert chunk * bound < 1 << 23
    for seed in GPU_SEEDS:
        worst_a = worst_b = worst_p = 0.0
        for v in range(16):
            a, b = operands(form, seed, v)
            worst_a = max(worst_a, float(np.abs(a).max()))
            worst_b = max(worst_b, float(np.abs(b).max()))
            worst_p = max(worst_p, float(np.abs(product(form, seed, v)).max()))
        print(form, "seed", hex(seed), "max |A|", worst_a, "max |B|", worst_b,
              "max |P|", worst_p)
        assert worst_a <= max_a and worst_b <= max_b and worst_p <= bound


@pytest.mark.parametrize("form", NEW_FORMS)
def test_the_model_notices_steps_variants_weights_and_scales(form):
    seed, iters = 0x5EED, 5
    right = model_checksum(form, 2, iters, seed)
    assert right == cotenancy.mfma_checksum(2, iters, seed, form)
    assert model_checksum(form, 2, iters, seed, drop_step_in_wave=3) != right
    assert model_checksum(form, 2, iters, seed, shift_wave=6) != right
    assert model_checksum(form, 2, iters, seed, swap_mn=True) != right
    if form in SCALED_FORMS:  # one scale bit of one row's second block, variant 0
        assert model_checksum(form, 2, iters, seed, flip=(37, 1)) != right


# --- fake children ------------------------------------------------------------

def flag(argv, name):
    return argv[argv.index(name) + 1]


class FakeChild:
    """Speaks the child protocol: READY, waits for GO, then its ending."""

    def __init__(self, argv, env, result=None, code=0):
        self.argv, self.env = list(argv), dict(env)
        self.kind = flag(argv, "--kind")
        self.form = flag(argv, "--form") if "--form" in argv else None
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


def answer(argv, rate=None, clock=SOLO_CLOCK, wrong=False, computes=None):
    """What a child given `argv` would print: `launches` back-to-back
    launches of 1000 ticks of a 100 MHz clock, and the checksum of its kind;
    an mfma child that of the form it was started with (bf16 without --form),
    or of `computes` when it runs another form than it was told to."""
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
        form = flag(argv, "--form") if "--form" in argv else "bf16"
        iters = int(flag(argv, "--iters")) or RULES[form][4]
        ticks = 999 * WORKGROUPS
        for l in out["launches"]:
            l.update(cycles=int(clock * 10 * ticks), ticks=ticks, clock_ghz=clock)
        out.update(form=form, iters=iters, clock_ghz=clock,
                   checksum=cotenancy.mfma_checksum(
                       WORKGROUPS, iters, seed, computes or form) ^ wrong)
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


# --- run_pair -------------------------------------------------------------------

def test_run_pair_gives_a_child_its_form_only_when_one_is_named():
    spawn = Spawner()
    run = run_pair(0, [{"mask": LOW, "kind": "mfma"}, {"mask": HIGH, "kind": "stream"}],
                   seed=7, spawn=spawn)
    assert run["ok"]
    assert all("--form" not in c.argv for c in spawn.log)
    assert spawn.log[0].argv[-2:] == ["--seed", "7"]  # today's argv, flag for flag

    spawn = Spawner()
    run = run_pair(0, [{"mask": LOW, "kind": "mfma"}, {"mask": HIGH, "kind": "stream"}],
                   seed=7, form="mxfp8", spawn=spawn)
    assert run["ok"]
    assert spawn.log[0].argv[-4:] == ["--seed", "7", "--form", "mxfp8"]
    assert "--form" not in spawn.log[1].argv  # the call-wide form is the mfma kind's
    assert run["tenants"][0]["form"] == "mxfp8"

    spawn = Spawner()
    run = run_pair(0, [{"mask": LOW, "form": "bf16"}, {"mask": HIGH, "form": "mxfp4"}],
                   ["mfma", "mfma"], form="fp8", spawn=spawn)
    assert run["ok"]  # a tenant's own form goes before the call's
    assert [c.form for c in spawn.log] == ["bf16", "mxfp4"]
    assert spawn.log[0].argv[-2:] == ["--form", "bf16"]

    spawn = Spawner()
    run = run_pair(0, [{"mask": LOW, "kind": "mfma"}, {"mask": HIGH, "kind": "mfma",
                                                     "form": "mxfp4"}], spawn=spawn)
    assert run["ok"] and [c.form for c in spawn.log] == [None, "mxfp4"]


def test_run_pair_refuses_a_misplaced_or_unknown_form_before_spawning():
    spawn = Spawner()
    with pytest.raises(ValueError, match="form"):
        run_pair(0, [{"mask": LOW, "kind": "mfma"},
                     {"mask": HIGH, "kind": "stream", "form": "fp8"}], spawn=spawn)
    with pytest.raises(ValueError, match="form"):
        run_pair(0, [{"mask": LOW, "form": "bf16"}], ["fma"], spawn=spawn)
    for bad in ("fp4", "MXFP4", ""):
        with pytest.raises(ValueError, match="mxfp4"):
            run_pair(0, [{"mask": LOW, "kind": "mfma"}], form=bad, spawn=spawn)
        with pytest.raises(ValueError, match="mxfp4"):
            run_pair(0, [{"mask": LOW, "kind": "mfma"},
                         {"mask": HIGH, "kind": "mfma", "form": bad}], spawn=spawn)
        with pytest.raises(ValueError, match="mxfp4"):  # even with no mfma tenant
            run_pair(0, [{"mask": LOW, "kind": "fma"}], form=bad, spawn=spawn)
    assert spawn.log == []


def test_child_parser_takes_a_form():
    p = cotenancy._child_parser()
    assert p.parse_args(["--child"]).form == "bf16"
    args = p.parse_args(["--child", "--kind", "mfma", "--form", "mxfp4"])
    assert (args.kind, args.form) == ("mfma", "mxfp4")
    with pytest.raises(SystemExit):
        p.parse_args(["--child", "--kind", "mfma", "--form", "fp4"])


def test_child_passes_the_form_to_both_runs(monkeypatch):
    import io

    from elastic_gpu_scheduler_amd import _native

    calls = []

    class Probe:
        def cu_tenant_run(self, device, mask, **kw):
            calls.append(kw)
            return {"kind": kw["kind"], "launches": []}

    monkeypatch.setattr(_native, "gpuprobe", lambda: Probe())
    out = io.StringIO()
    argv = ["--child", "--kind", "mfma", "--launches", "5", "--form", "mxfp8"]
    assert cotenancy.child_main(argv, stdin=io.StringIO("GO\n"), stdout=out) == 0
    assert [c["form"] for c in calls] == ["mxfp8", "mxfp8"]
    assert [c["launches"] for c in calls] == [1, 5]


# --- isolation_report -----------------------------------------------------------

def test_report_runs_every_mfma_tenant_with_the_call_s_form():
    spawn = Spawner()
    report = isolation_report(0, TENANTS, pairs=cotenancy.MFMA_PAIRS, seed=0x5EED,
                              form="mxfp4", spawn=spawn, expected_checksum=checksum_of)
    assert report["ok"], report
    assert len(spawn.log) == 13
    for c in spawn.log:
        assert c.form == ("mxfp4" if c.kind == "mfma" else None)
    for i in range(2):
        assert report["solo"][i]["mfma"]["form"] == "mxfp4"
        assert "form" not in report["solo"][i]["stream"]
    for pair in report["pairs"].values():
        for t in pair["tenants"]:
            assert t.get("form") == ("mxfp4" if t["kind"] == "mfma" else None)
            assert t["ratio"] == 1.0


def test_report_without_a_form_starts_and_reports_as_before():
    spawn = Spawner()
    report = isolation_report(0, TENANTS, pairs=cotenancy.MFMA_PAIRS, spawn=spawn,
                              expected_checksum=checksum_of)
    assert report["ok"], report
    assert all("--form" not in c.argv for c in spawn.log)
    assert all("form" not in report["solo"][i]["mfma"] for i in range(2))
    assert all("form" not in t for p in report["pairs"].values() for t in p["tenants"])


def test_report_honours_each_tenant_s_own_form_solo_and_paired():
    """A bf16 tenant beside an mxfp4 one: children 0 and 1 are the solo
    runs, 2 and 3 the pair."""
    spawn = Spawner()
    tenants = [{"mask": LOW, "form": "bf16"}, {"mask": HIGH, "form": "mxfp4"}]
    report = isolation_report(0, tenants, pairs=[("mfma", "mfma")], spawn=spawn)
    assert report["ok"], report
    assert [c.form for c in spawn.log] == ["bf16", "mxfp4", "bf16", "mxfp4"]
    assert [report["solo"][i]["mfma"]["form"] for i in range(2)] == ["bf16", "mxfp4"]
    assert [t["form"] for t in report["pairs"]["mfma/mfma"]["tenants"]] == ["bf16", "mxfp4"]
    # one tenant's own form beside the call's
    spawn = Spawner()
    report = isolation_report(0, [{"mask": LOW}, {"mask": HIGH, "form": "mxfp4"}],
                              pairs=[("mfma", "mfma"), ("stream", "mfma")], form="fp8",
                              spawn=spawn, expected_checksum=checksum_of)
    assert report["ok"], report
    assert [(c.kind, c.form) for c in spawn.log] == [
        ("stream", None), ("mfma", "fp8"), ("mfma", "mxfp4"),
        ("mfma", "fp8"), ("mfma", "mxfp4"), ("stream", None), ("mfma", "mxfp4")]
    assert report["pairs"]["stream/mfma"]["tenants"][1]["form"] == "mxfp4"
    assert "form" not in report["pairs"]["stream/mfma"]["tenants"][0]


def test_report_holds_a_checksum_against_the_tenant_s_own_form():
    tenants = [{"mask": LOW, "form": "bf16"}, {"mask": HIGH, "form": "mxfp4"}]

    def script(n, argv, env):  # child 3, the mxfp4 tenant of the pair, is off by one
        return FakeChild(argv, env, answer(argv, wrong=(n == 3)))

    report = isolation_report(0, tenants, pairs=[("mfma", "mfma")], spawn=Spawner(script))
    assert not report["ok"] and report["reason"] == "bad-checksum"
    pair = report["pairs"]["mfma/mfma"]
    assert pair["tenants"][1]["reason"] == "bad-checksum"
    assert "reason" not in pair["tenants"][0]

    def script(n, argv, env):  # the mxfp4 tenant hands in the bf16 checksum, solo
        return FakeChild(argv, env, answer(argv, computes="bf16" if n == 1 else None))

    report = isolation_report(0, tenants, pairs=[("mfma", "mfma")], spawn=Spawner(script))
    assert not report["ok"] and report["reason"] == "bad-checksum"
    assert report["pairs"]["mfma/mfma"]["ok"]  # the pair's own children were right

    def script(n, argv, env):  # every child ignores its form
        return FakeChild(argv, env, answer(argv, computes="bf16"))

    report = isolation_report(0, TENANTS, pairs=[("mfma", "mfma")], form="mxfp8",
                              spawn=Spawner(script))
    assert not report["ok"] and report["reason"] == "bad-checksum"


def test_report_refuses_an_unknown_form_before_spawning():
    spawn = Spawner()
    with pytest.raises(ValueError, match="mxfp4"):
        isolation_report(0, TENANTS, pairs=cotenancy.MFMA_PAIRS, form="fp6", spawn=spawn)
    with pytest.raises(ValueError, match="mxfp4"):
        isolation_report(0, [{"mask": LOW}, {"mask": HIGH, "form": "bf8"}],
                         pairs=cotenancy.MFMA_PAIRS, spawn=spawn)
    assert spawn.log == []


# --- agent and CLI --------------------------------------------------------------

def stub_layouts(monkeypatch, layout=LAYOUT, cards=1):
    monkeypatch.setattr(NodeAgent, "mask_layouts",
                        lambda self: {i: dict(layout) for i in range(cards)})


def test_agent_parser_co_tenancy_mfma_form():
    from elastic_gpu_scheduler_amd.cmd.agent_main import build_parser

    p = build_parser()
    args = p.parse_args(["--co-tenancy", "--co-tenancy-mfma"])
    assert args.co_tenancy_mfma is True and args.co_tenancy_mfma_form is None
    args = p.parse_args(["--co-tenancy", "--co-tenancy-mfma",
                         "--co-tenancy-mfma-form", "mxfp4"])
    assert args.co_tenancy_mfma_form == ("mxfp4",)
    args = p.parse_args(["--co-tenancy", "--co-tenancy-mfma",
                         "--co-tenancy-mfma-form", "bf16,fp8,mxfp8,mxfp4"])
    assert args.co_tenancy_mfma_form == FORMS
    for bad in ("fp4", "mxfp4,", "mxfp8,fp6", ""):
        with pytest.raises(SystemExit):
            p.parse_args(["--co-tenancy", "--co-tenancy-mfma",
                          "--co-tenancy-mfma-form", bad])
    with pytest.raises(SystemExit):  # it takes a value
        p.parse_args(["--co-tenancy", "--co-tenancy-mfma", "--co-tenancy-mfma-form"])


def test_agent_main_mfma_form_reports_every_card_and_form_in_turn(monkeypatch, capsys):
    from elastic_gpu_scheduler_amd.cmd import agent_main

    stub_layouts(monkeypatch, cards=2)
    calls = []

    def verify(self, card, shares, **kw):
        calls.append((card, shares, kw))
        return {"ok": True, "n": len(calls)}

    monkeypatch.setattr(NodeAgent, "verify_isolation", verify)
    assert agent_main.main(["--co-tenancy", "25,75", "--co-tenancy-mfma",
                            "--co-tenancy-mfma-form", "fp8,mxfp4"]) == 0
    pairs = cotenancy.MFMA_PAIRS
    assert calls == [(0, (25, 75), {"pairs": pairs, "form": "fp8"}),
                     (0, (25, 75), {"pairs": pairs, "form": "mxfp4"}),
                     (1, (25, 75), {"pairs": pairs, "form": "fp8"}),
                     (1, (25, 75), {"pairs": pairs, "form": "mxfp4"})]
    assert json.loads(capsys.readouterr().out) == {
        "0": {"fp8": {"ok": True, "n": 1}, "mxfp4": {"ok": True, "n": 2}},
        "1": {"fp8": {"ok": True, "n": 3}, "mxfp4": {"ok": True, "n": 4}}}
    # without --co-tenancy-mfma the flag measures nothing
    del calls[:]
    for argv in (["--co-tenancy-mfma-form", "fp8"],
                 ["--co-tenancy", "--co-tenancy-mfma-form", "fp8"]):
        assert agent_main.main(argv) == 2
        out, err = capsys.readouterr()
        assert calls == [] and out == "" and "--co-tenancy-mfma" in err


def test_agent_verify_isolation_passes_the_form_through(monkeypatch):
    stub_layouts(monkeypatch)
    spawn = Spawner()
    report = NodeAgent("n").verify_isolation(0, (50, 50), pairs=cotenancy.MFMA_PAIRS,
                                             form="mxfp8", spawn=spawn,
                                             expected_checksum=checksum_of)
    assert report["ok"], report
    assert {c.form for c in spawn.log if c.kind == "mfma"} == {"mxfp8"}
    assert report["solo"][0]["mfma"]["form"] == "mxfp8"
    doc = NodeAgent.verify_isolation.__doc__
    assert "form" in doc and all(f in doc for f in FORMS)


# --- binding argument checks ------------------------------------------------

@needs_probe
def test_form_is_checked_before_the_device_is_touched():
    p = gpuprobe()
    for bad in ("fp4", "MXFP4", "mxfp4 ", ""):
        with pytest.raises(ValueError) as exc:
            p.cu_tenant_run(0, kind="mfma", form=bad)
        assert all(f in str(exc.value) for f in FORMS)
    for kind in ("fma", "stream", "cache", "chase"):
        for form in NEW_FORMS:
            with pytest.raises(ValueError, match="mfma"):
                p.cu_tenant_run(0, kind=kind, form=form)
    doc = p.cu_tenant_run.__doc__
    assert all(f in doc for f in FORMS)
    assert "form" in doc and "e4m3" in doc and "e2m1" in doc and "E8M0" in doc


@needs_probe
def test_forms_raise_without_device():
    import torch

    if torch.cuda.is_available():
        return  # a device is visible: covered by the gpu-marked tests
    p = gpuprobe()
    for form in FORMS:
        with pytest.raises(RuntimeError):  # TypeError while there is no form
            p.cu_tenant_run(0, kind="mfma", launches=1, iters=1, form=form)
    with pytest.raises(RuntimeError):  # bf16 goes with every kind
        p.cu_tenant_run(0, kind="fma", form="bf16")
