"""The mfma tenant with its operands re-read from LDS (operands="lds"), the
parts that need no GPU: the closed-form oracle of every form against a
brute-force model of the kernel written from the rule alone (the workgroup's
LDS image laid out slot by slot, every wave walking its steps through the
rotating slots in chunks, integer matrices, the register weights), the
cross-check values computed for the feature, one step against registers,
that nothing moves when no operands are named, `operands` on its way through
run_pair, isolation_report, the child and the CLI over (fake) children, and
the binding's argument checks.

The operand rules, the weights and the fake children are those of
test_mfma_forms_cpu.py."""
from __future__ import annotations

import io
import json

import numpy as np
import pytest

from elastic_gpu_scheduler_amd._native import gpuprobe, gpuprobe_available
from elastic_gpu_scheduler_amd.agent import cotenancy
from elastic_gpu_scheduler_amd.agent.agent import NodeAgent
from elastic_gpu_scheduler_amd.agent.cotenancy import isolation_report, run_pair
from tests import test_mfma_forms_cpu as forms_cpu
from tests.test_mfma_forms_cpu import (FORMS, HIGH, LOW, RULES, TENANTS, WORKGROUPS,
                                       FakeChild, Spawner, checksum_of, flag,
                                       stub_layouts)

needs_probe = pytest.mark.skipif(not gpuprobe_available(),
                                 reason="_gpuprobe extension not built")

MASK64 = (1 << 64) - 1
STEP_BYTES = {"bf16": 4096, "fp8": 2048, "mxfp8": 9216, "mxfp4": 5120}


# --- a brute-force model of the kernel ------------------------------------------

_MATRICES = {}


def matrices(form, seed, variant):
    """Integer A (64 x K) and B (K x 64) of one variant."""
    key = (form, seed & 0xFFFFFFFF, variant)
    if key not in _MATRICES:
        a, b = forms_cpu.operands(form, seed, variant)
        assert (a == np.round(a)).all() and (b == np.round(b)).all()
        _MATRICES[key] = (a.astype(np.int64), b.astype(np.int64))
    return _MATRICES[key]


def lds_image(form, seed, workgroup):
    """What a workgroup's LDS holds once the fill is closed: slot j is what
    the workgroup's wave j built, the fragments of variant (4 b + j) % 16."""
    return [matrices(form, seed, (4 * workgroup + j) % 16) for j in range(4)]


def model_checksum(form, workgroups, iters, seed, *, rotate=True):
    """Every wave walks its steps in chunks: at step i of the launch, counted
    across chunks, global wave w multiplies what lies in slot (w + i) & 3 of
    its workgroup's image into its tile, which starts a chunk from zero and
    is folded, with the register weights, at the chunk's end. Every lane's
    fold weighted by its global index, modulo 2^64 as on the device.
    `rotate=False` is a kernel that stays on its own slot."""
    weight, owner = forms_cpu.weights()
    chunk = RULES[form][3]
    total = 0
    for b in range(workgroups):
        image = lds_image(form, seed, b)
        for j in range(4):
            w = 4 * b + j
            fold = [0] * 64
            done = 0
            while done < iters:
                steps = min(chunk, iters - done)
                acc = np.zeros((64, 64), dtype=np.int64)
                for i in range(done, done + steps):
                    a, bm = image[(w + i) & 3 if rotate else j]
                    acc += a @ bm
                    assert np.abs(acc).max() < 1 << 23  # exact in f32
                contrib = acc * weight
                for lane in range(64):
                    fold[lane] = (fold[lane] + int(contrib[owner == lane].sum())) & MASK64
                done += steps
            for lane in range(64):
                total = (total + (64 * w + lane + 1) * fold[lane]) & MASK64
    return total


@pytest.mark.parametrize("workgroups", (1, 5))
@pytest.mark.parametrize("form", FORMS)
def test_lds_checksum_equals_the_brute_force_model(form, workgroups):
    """5 workgroups are 20 waves: the 16 variants wrap. 1, 2, 3, 5 and 7
    steps leave every remainder of the rotation."""
    for iters in (1, 2, 3, 5, 7):
        got = cotenancy.mfma_checksum(workgroups, iters, 0x5EED, form, operands="lds")
        assert 0 <= got < 1 << 64
        assert got == model_checksum(form, workgroups, iters, 0x5EED), (
            form, workgroups, iters)


def test_the_model_notices_a_kernel_that_does_not_rotate():
    for form in FORMS:
        assert model_checksum(form, 1, 2, 0x5EED, rotate=False) != model_checksum(
            form, 1, 2, 0x5EED)
        assert model_checksum(form, 1, 2, 0x5EED, rotate=False) == (
            cotenancy.mfma_checksum(1, 2, 0x5EED, form))


CROSS_CHECK = {  # seed 0x5EED, (workgroups, iters): computed from the rule for the feature
    "bf16": {(5, 2): 3612190252, (8, 3): 15340503074, (5, 7): 14031466970,
             (3, 2051): 2983140262561},
    "fp8": {(5, 2): 18446744068949836676, (8, 3): 18446744072827977536,
            (5, 7): 18446744055685146382, (3, 2051): 18446743709134055197},
    "mxfp8": {(5, 2): 18446744068676079802, (8, 3): 18446744026854864820,
              (5, 7): 18446744056058186603, (3, 2051): 18446741177960666621},
    "mxfp4": {(5, 2): 14350696694, (8, 3): 55748185392, (5, 7): 48718291389,
              (3, 2051): 4827477490429},
}


@pytest.mark.parametrize("form", FORMS)
def test_the_cross_check_values(form):
    for (workgroups, iters), want in CROSS_CHECK[form].items():
        assert cotenancy.mfma_checksum(workgroups, iters, 0x5EED, form, "lds") == want, (
            form, workgroups, iters)


def test_the_cross_check_value_of_a_whole_card():
    """bf16, seed 1, 2048 workgroups, 4 steps: every slot once."""
    assert cotenancy.mfma_checksum(2048, 4, 1, "bf16", "lds") == 457915218780160
    assert cotenancy.mfma_checksum(2048, 4, 1, "bf16", "registers") == 457709101834240
    assert cotenancy.mfma_checksum(2048, 4, 1) == 457709101834240


@pytest.mark.parametrize("form", FORMS)
def test_one_step_is_the_wave_s_own_variant(form):
    for workgroups, seed in ((1, 0x5EED), (5, 0x5EED), (1024, 1)):
        assert cotenancy.mfma_checksum(workgroups, 1, seed, form, "lds") == (
            cotenancy.mfma_checksum(workgroups, 1, seed, form, "registers"))
        assert cotenancy.mfma_checksum(workgroups, 2, seed, form, "lds") != (
            cotenancy.mfma_checksum(workgroups, 2, seed, form, "registers"))
    assert cotenancy.mfma_checksum(1, 1, 0x5EED, "bf16", "lds") == 121685947


def test_registers_are_the_default_and_are_unchanged():
    for form in FORMS:
        for args in ((2, 3, 0x5EED), (1024, 2049, 1), (5, 4099, 0x1_0000_0007)):
            assert cotenancy.mfma_checksum(*args, form, operands="registers") == (
                cotenancy.mfma_checksum(*args, form))
    assert cotenancy.mfma_checksum(2, 3, 0x5EED) == 1473222840
    assert cotenancy.mfma_checksum(2, 3, 0x5EED, "mxfp4", "registers") == 4158640977
    assert cotenancy.mfma_checksum(1024, 2049, 1, operands="registers",
                                   form="fp8") == 18409058969200509184


def test_operands_and_their_table():
    assert cotenancy.MFMA_OPERANDS == ("registers", "lds")
    assert cotenancy.MFMA_LDS_SLOTS == 4
    assert cotenancy.MFMA_LDS_STEP_BYTES == STEP_BYTES
    # Planes of 64 lanes x 16 bytes: A0, A1, B0, B1 of K elements per row, fp8
    # two fragments to a plane, and one plane of scales for the scaled forms.
    bits = {"bf16": 16, "fp8": 8, "mxfp8": 8, "mxfp4": 4}
    for form in FORMS:
        fragments = 4 * 32 * RULES[form][1] * bits[form] // 8
        scales = 1024 if form in ("mxfp8", "mxfp4") else 0
        assert STEP_BYTES[form] == fragments + scales
        assert 4 * STEP_BYTES[form] <= 160 << 10
    for bad in ("LDS", "shared", "", None, 1):
        with pytest.raises(ValueError, match="registers, lds"):
            cotenancy.mfma_checksum(2, 3, 1, operands=bad)
    # nothing older moves
    assert cotenancy.KINDS == ("fma", "stream", "cache", "chase")
    assert cotenancy.ALL_KINDS == cotenancy.KINDS + ("mfma",)
    assert cotenancy.MFMA_PAIRS == (
        ("mfma", "mfma"), ("mfma", "stream"), ("stream", "mfma"), ("mfma", "fma"))
    assert cotenancy.MFMA_FORMS == FORMS


# --- fake children ------------------------------------------------------------

def operands_of(argv):
    return flag(argv, "--operands") if "--operands" in argv else None


def answer(argv, computes=None):
    """What a child given `argv` would print (test_mfma_forms_cpu.answer); an
    mfma child hands in the sum of the operands it was started with
    (registers without --operands), or of `computes` when it runs with
    others than it was told to, and reports as the probe does."""
    out = forms_cpu.answer(argv)
    if out["kind"] == "mfma":
        told = operands_of(argv) or "registers"
        out["checksum"] = cotenancy.mfma_checksum(
            WORKGROUPS, out["iters"], int(flag(argv, "--seed")), out["form"],
            computes or told)
        if told == "lds":
            out.update(operands="lds", lds_bytes=4 * STEP_BYTES[out["form"]],
                       lds_bytes_per_launch=4 * WORKGROUPS * out["iters"]
                       * STEP_BYTES[out["form"]])
    return out


def spawner(script=None):
    return Spawner(script or (lambda n, argv, env: FakeChild(argv, env, answer(argv))))


# --- run_pair -------------------------------------------------------------------

def test_run_pair_gives_a_child_its_operands_only_when_they_are_named():
    spawn = spawner()
    run = run_pair(0, [{"mask": LOW, "kind": "mfma"}, {"mask": HIGH, "kind": "stream"}],
                   seed=7, spawn=spawn)
    assert run["ok"]
    assert all("--operands" not in c.argv for c in spawn.log)
    assert spawn.log[0].argv[-2:] == ["--seed", "7"]  # today's argv, flag for flag

    spawn = spawner()
    run = run_pair(0, [{"mask": LOW, "kind": "mfma"}, {"mask": HIGH, "kind": "stream"}],
                   seed=7, operands="lds", spawn=spawn)
    assert run["ok"]
    assert spawn.log[0].argv[-4:] == ["--seed", "7", "--operands", "lds"]
    assert "--form" not in spawn.log[0].argv
    assert "--operands" not in spawn.log[1].argv  # the call-wide one is the mfma kind's
    assert run["tenants"][0]["operands"] == "lds"

    spawn = spawner()  # after --form
    run = run_pair(0, [{"mask": LOW, "kind": "mfma"}], seed=7, form="mxfp8",
                   operands="lds", spawn=spawn)
    assert run["ok"]
    assert spawn.log[0].argv[-6:] == ["--seed", "7", "--form", "mxfp8",
                                      "--operands", "lds"]

    spawn = spawner()  # a tenant's own goes before the call's
    run = run_pair(0, [{"mask": LOW, "operands": "registers"},
                       {"mask": HIGH, "operands": "lds", "form": "mxfp4"}],
                   ["mfma", "mfma"], operands="lds", form="fp8", spawn=spawn)
    assert run["ok"]
    assert [operands_of(c.argv) for c in spawn.log] == ["registers", "lds"]
    assert spawn.log[0].argv[-4:] == ["--form", "fp8", "--operands", "registers"]
    assert spawn.log[1].argv[-4:] == ["--form", "mxfp4", "--operands", "lds"]

    spawn = spawner()
    run = run_pair(0, [{"mask": LOW, "kind": "mfma"},
                       {"mask": HIGH, "kind": "mfma", "operands": "lds"}], spawn=spawn)
    assert run["ok"] and [operands_of(c.argv) for c in spawn.log] == [None, "lds"]


def test_run_pair_refuses_misplaced_or_unknown_operands_before_spawning():
    spawn = spawner()
    with pytest.raises(ValueError, match="operands"):
        run_pair(0, [{"mask": LOW, "kind": "mfma"},
                     {"mask": HIGH, "kind": "stream", "operands": "lds"}], spawn=spawn)
    with pytest.raises(ValueError, match="operands"):
        run_pair(0, [{"mask": LOW, "operands": "registers"}], ["fma"], spawn=spawn)
    for bad in ("LDS", "shared", ""):
        with pytest.raises(ValueError, match="registers, lds"):
            run_pair(0, [{"mask": LOW, "kind": "mfma"}], operands=bad, spawn=spawn)
        with pytest.raises(ValueError, match="registers, lds"):
            run_pair(0, [{"mask": LOW, "kind": "mfma"},
                         {"mask": HIGH, "kind": "mfma", "operands": bad}], spawn=spawn)
        with pytest.raises(ValueError, match="registers, lds"):  # even with no mfma tenant
            run_pair(0, [{"mask": LOW, "kind": "fma"}], operands=bad, spawn=spawn)
    assert spawn.log == []


def test_child_parser_takes_operands():
    p = cotenancy._child_parser()
    assert p.parse_args(["--child"]).operands is None
    args = p.parse_args(["--child", "--kind", "mfma", "--form", "mxfp4",
                         "--operands", "lds"])
    assert (args.kind, args.form, args.operands) == ("mfma", "mxfp4", "lds")
    assert p.parse_args(["--child", "--operands", "registers"]).operands == "registers"
    with pytest.raises(SystemExit):
        p.parse_args(["--child", "--kind", "mfma", "--operands", "shared"])


def run_child(monkeypatch, argv):
    from elastic_gpu_scheduler_amd import _native

    calls = []

    class Probe:
        def cu_tenant_run(self, device, mask, **kw):
            calls.append(kw)
            return {"kind": kw["kind"], "launches": []}

    monkeypatch.setattr(_native, "gpuprobe", lambda: Probe())
    out = io.StringIO()
    assert cotenancy.child_main(argv, stdin=io.StringIO("GO\n"), stdout=out) == 0
    return calls


def test_child_passes_the_operands_to_both_runs(monkeypatch):
    calls = run_child(monkeypatch, ["--child", "--kind", "mfma", "--launches", "5",
                                    "--form", "mxfp8", "--operands", "lds"])
    assert [c["operands"] for c in calls] == ["lds", "lds"]
    assert [c["form"] for c in calls] == ["mxfp8", "mxfp8"]
    assert [c["launches"] for c in calls] == [1, 5]
    calls = run_child(monkeypatch, ["--child", "--kind", "mfma", "--launches", "5"])
    assert len(calls) == 2 and all("operands" not in c for c in calls)
    # beside another kind it is handed on, so that the probe refuses it
    calls = run_child(monkeypatch, ["--child", "--kind", "fma", "--operands", "lds"])
    assert [c["operands"] for c in calls] == ["lds", "lds"]


# --- isolation_report -----------------------------------------------------------

def test_report_runs_every_mfma_tenant_with_the_call_s_operands():
    spawn = spawner()
    report = isolation_report(0, TENANTS, pairs=cotenancy.MFMA_PAIRS, seed=0x5EED,
                              iters=6, operands="lds", spawn=spawn,
                              expected_checksum=checksum_of)
    assert report["ok"], report
    assert len(spawn.log) == 13
    for c in spawn.log:
        assert operands_of(c.argv) == ("lds" if c.kind == "mfma" else None)
        assert "--form" not in c.argv
    for i in range(2):
        assert report["solo"][i]["mfma"]["operands"] == "lds"
        assert "form" not in report["solo"][i]["mfma"]
        assert "operands" not in report["solo"][i]["stream"]
    for pair in report["pairs"].values():
        for t in pair["tenants"]:
            assert t.get("operands") == ("lds" if t["kind"] == "mfma" else None)
            assert t["ratio"] == 1.0


def test_report_without_operands_starts_and_reports_as_before():
    spawn = spawner()
    report = isolation_report(0, TENANTS, pairs=cotenancy.MFMA_PAIRS, form="mxfp4",
                              spawn=spawn, expected_checksum=checksum_of)
    assert report["ok"], report
    assert all("--operands" not in c.argv for c in spawn.log)
    assert all("operands" not in report["solo"][i]["mfma"] for i in range(2))
    assert all("operands" not in t for p in report["pairs"].values()
               for t in p["tenants"])


def test_report_honours_each_tenant_s_own_operands_solo_and_paired():
    """A tenant from registers beside one from LDS: children 0 and 1 are the
    solo runs, 2 and 3 the pair."""
    spawn = spawner()
    tenants = [{"mask": LOW, "operands": "registers"},
               {"mask": HIGH, "operands": "lds", "form": "mxfp4"}]
    report = isolation_report(0, tenants, pairs=[("mfma", "mfma")], iters=5,
                              spawn=spawn)
    assert report["ok"], report
    assert [operands_of(c.argv) for c in spawn.log] == ["registers", "lds"] * 2
    assert [c.form for c in spawn.log] == [None, "mxfp4"] * 2
    assert [report["solo"][i]["mfma"]["operands"] for i in range(2)] == [
        "registers", "lds"]
    assert [t["operands"] for t in report["pairs"]["mfma/mfma"]["tenants"]] == [
        "registers", "lds"]
    # one tenant's own beside the call's
    spawn = spawner()
    report = isolation_report(0, [{"mask": LOW}, {"mask": HIGH, "operands": "registers"}],
                              pairs=[("mfma", "mfma"), ("stream", "mfma")],
                              operands="lds", iters=5, spawn=spawn,
                              expected_checksum=checksum_of)
    assert report["ok"], report
    assert [(c.kind, operands_of(c.argv)) for c in spawn.log] == [
        ("stream", None), ("mfma", "lds"), ("mfma", "registers"),
        ("mfma", "lds"), ("mfma", "registers"), ("stream", None), ("mfma", "registers")]
    assert report["pairs"]["stream/mfma"]["tenants"][1]["operands"] == "registers"
    assert "operands" not in report["pairs"]["stream/mfma"]["tenants"][0]


def test_report_holds_a_checksum_against_the_tenant_s_own_operands():
    def script(n, argv, env):  # child 3, asked for LDS in the pair, sums as from registers
        return FakeChild(argv, env, answer(argv, computes="registers" if n == 3 else None))

    report = isolation_report(0, TENANTS, pairs=[("mfma", "mfma")], iters=2,
                              operands="lds", spawn=Spawner(script))
    assert not report["ok"] and report["reason"] == "bad-checksum"
    pair = report["pairs"]["mfma/mfma"]
    assert pair["tenants"][1]["reason"] == "bad-checksum"
    assert "reason" not in pair["tenants"][0]

    def script(n, argv, env):  # the same, alone
        return FakeChild(argv, env, answer(argv, computes="registers" if n == 1 else None))

    tenants = [{"mask": LOW}, {"mask": HIGH, "operands": "lds"}]
    report = isolation_report(0, tenants, pairs=[("mfma", "mfma")], iters=7,
                              form="mxfp8", spawn=Spawner(script))
    assert not report["ok"] and report["reason"] == "bad-checksum"
    assert report["pairs"]["mfma/mfma"]["ok"]  # the pair's own children were right

    def script(n, argv, env):  # a child that read from LDS though nobody asked
        return FakeChild(argv, env, answer(argv, computes="lds"))

    report = isolation_report(0, TENANTS, pairs=[("mfma", "mfma")], iters=2,
                              spawn=Spawner(script))
    assert not report["ok"] and report["reason"] == "bad-checksum"
    # with one step per launch the two sums are equal, and so nothing is seen
    report = isolation_report(0, TENANTS, pairs=[("mfma", "mfma")], iters=1,
                              spawn=Spawner(script))
    assert report["ok"], report


def test_report_refuses_unknown_operands_before_spawning():
    spawn = spawner()
    with pytest.raises(ValueError, match="registers, lds"):
        isolation_report(0, TENANTS, pairs=cotenancy.MFMA_PAIRS, operands="shared",
                         spawn=spawn)
    with pytest.raises(ValueError, match="registers, lds"):
        isolation_report(0, [{"mask": LOW}, {"mask": HIGH, "operands": "LDS"}],
                         pairs=cotenancy.MFMA_PAIRS, spawn=spawn)
    assert spawn.log == []


# --- agent and CLI --------------------------------------------------------------

def test_agent_parser_co_tenancy_mfma_operands():
    from elastic_gpu_scheduler_amd.cmd.agent_main import build_parser

    p = build_parser()
    args = p.parse_args(["--co-tenancy", "--co-tenancy-mfma"])
    assert args.co_tenancy_mfma_operands is None
    for value in ("registers", "lds"):
        args = p.parse_args(["--co-tenancy", "--co-tenancy-mfma",
                             "--co-tenancy-mfma-operands", value])
        assert args.co_tenancy_mfma_operands == value
    args = p.parse_args(["--co-tenancy", "--co-tenancy-mfma", "--co-tenancy-mfma-form",
                         "fp8,mxfp4", "--co-tenancy-mfma-operands", "lds"])
    assert args.co_tenancy_mfma_form == ("fp8", "mxfp4")
    assert args.co_tenancy_mfma_operands == "lds"
    for bad in ("LDS", "shared", "registers,lds", ""):
        with pytest.raises(SystemExit):
            p.parse_args(["--co-tenancy", "--co-tenancy-mfma",
                          "--co-tenancy-mfma-operands", bad])
    with pytest.raises(SystemExit):  # it takes a value
        p.parse_args(["--co-tenancy", "--co-tenancy-mfma", "--co-tenancy-mfma-operands"])


def test_agent_main_mfma_operands(monkeypatch, capsys):
    from elastic_gpu_scheduler_amd.cmd import agent_main

    stub_layouts(monkeypatch, cards=2)
    calls = []

    def verify(self, card, shares, **kw):
        calls.append((card, shares, kw))
        return {"ok": True, "n": len(calls)}

    monkeypatch.setattr(NodeAgent, "verify_isolation", verify)
    pairs = cotenancy.MFMA_PAIRS
    assert agent_main.main(["--co-tenancy", "25,75", "--co-tenancy-mfma",
                            "--co-tenancy-mfma-operands", "lds"]) == 0
    assert calls == [(0, (25, 75), {"pairs": pairs, "operands": "lds"}),
                     (1, (25, 75), {"pairs": pairs, "operands": "lds"})]
    assert json.loads(capsys.readouterr().out) == {
        "0": {"ok": True, "n": 1}, "1": {"ok": True, "n": 2}}  # today's shape
    del calls[:]
    assert agent_main.main(["--co-tenancy", "--co-tenancy-mfma", "--co-tenancy-mfma-form",
                            "fp8,mxfp4", "--co-tenancy-mfma-operands", "lds"]) == 0
    assert calls == [
        (card, (50, 50), {"pairs": pairs, "form": form, "operands": "lds"})
        for card in (0, 1) for form in ("fp8", "mxfp4")]
    assert json.loads(capsys.readouterr().out) == {
        "0": {"fp8": {"ok": True, "n": 1}, "mxfp4": {"ok": True, "n": 2}},
        "1": {"fp8": {"ok": True, "n": 3}, "mxfp4": {"ok": True, "n": 4}}}
    # without the flag nothing is handed on
    del calls[:]
    assert agent_main.main(["--co-tenancy", "--co-tenancy-mfma"]) == 0
    assert calls == [(0, (50, 50), {"pairs": pairs}), (1, (50, 50), {"pairs": pairs})]
    capsys.readouterr()
    # without --co-tenancy-mfma the flag measures nothing
    del calls[:]
    for argv in (["--co-tenancy-mfma-operands", "lds"],
                 ["--co-tenancy", "--co-tenancy-mfma-operands", "lds"],
                 ["--co-tenancy", "--co-tenancy-chase",
                  "--co-tenancy-mfma-operands", "registers"]):
        assert agent_main.main(argv) == 2
        out, err = capsys.readouterr()
        assert calls == [] and out == "" and "--co-tenancy-mfma" in err


def test_agent_verify_isolation_passes_the_operands_through(monkeypatch):
    stub_layouts(monkeypatch)
    spawn = spawner()
    report = NodeAgent("n").verify_isolation(0, (50, 50), pairs=cotenancy.MFMA_PAIRS,
                                             form="mxfp8", operands="lds", iters=6,
                                             spawn=spawn, expected_checksum=checksum_of)
    assert report["ok"], report
    assert {operands_of(c.argv) for c in spawn.log if c.kind == "mfma"} == {"lds"}
    assert report["solo"][0]["mfma"]["operands"] == "lds"
    assert report["solo"][0]["mfma"]["form"] == "mxfp8"
    doc = NodeAgent.verify_isolation.__doc__
    assert "operands" in doc and "registers" in doc and "lds" in doc


# --- binding argument checks ------------------------------------------------

@needs_probe
def test_operands_are_checked_before_the_device_is_touched():
    p = gpuprobe()
    for bad in ("LDS", "shared", "lds ", ""):
        with pytest.raises(ValueError) as exc:
            p.cu_tenant_run(0, kind="mfma", operands=bad)
        assert "registers" in str(exc.value) and "lds" in str(exc.value)
    for kind in ("fma", "stream", "cache", "chase"):
        with pytest.raises(ValueError, match="mfma"):
            p.cu_tenant_run(0, kind=kind, operands="lds")
    with pytest.raises(ValueError, match="kind must be"):  # the kind's text is unchanged
        p.cu_tenant_run(0, kind="lds", operands="lds")
    doc = p.cu_tenant_run.__doc__
    assert "operands" in doc and "lds_bytes_per_launch" in doc and "ds_read_b128" in doc
    for nbytes in STEP_BYTES.values():
        assert str(nbytes) in doc


@needs_probe
def test_operands_raise_without_device():
    import torch

    if torch.cuda.is_available():
        return  # a device is visible: covered by the gpu-marked tests
    p = gpuprobe()
    for operands in ("registers", "lds"):
        for form in FORMS:
            with pytest.raises(RuntimeError):  # TypeError while there are no operands
                p.cu_tenant_run(0, kind="mfma", launches=1, iters=1, form=form,
                                operands=operands)
    with pytest.raises(RuntimeError):  # registers go with every kind
        p.cu_tenant_run(0, kind="fma", operands="registers")
