"""Two tenants on one card at once: does a gpu-core share keep its rate while
the neighbour runs? (No GPU import at module level.)

Each tenant is a fresh child process started the way a container is wired:
the inherited environment plus ROC_GLOBAL_CU_MASK. A child runs the probe's
cu_tenant_run, whose launches are stamped with the card's constant-rate wall
clock. That clock is the same for every process on the card, so the parent
can lay the two children's launches side by side afterwards and keep only
those that provably ran while the other tenant was running:

  * overlap()          — per launch of A, the fraction covered by B's launches;
  * run_pair()         — up to two children at once, READY / GO handshake;
  * isolation_report() — solo rates first, then the pairs, then the ratios;
  * cache_profile()    — one tenant alone, its rate by working-set size;
  * chase_profile()    — one tenant alone, its time per dependent load by
                         working-set size.

A tenant is one of four kinds: "fma" (registers only), "stream" (1 GiB read
through, non-temporal), "cache" (a working set re-read with plain loads,
every byte of it live for the whole launch) or "chase" (every wave follows a
chain of dependent loads, one 128-byte line in flight at a time: bound by
latency, not by bandwidth). Each kind may be given a window of its own, so a
12 MiB cache tenant can sit next to a 1 GiB streamer.

The chase tenant's oracle is here and in closed form: chase_stride() and
chase_checksum() state where every wave must end, in integers only.

A fifth kind, "mfma", loads the matrix cores: every wave issues bf16 MFMAs
back to back on operands it keeps in registers. It is kept apart from KINDS
(MATRIX_KINDS, ALL_KINDS) because it is the one kind a CU mask cannot be
expected to isolate: the chip lowers its shader clock under matrix load, and
that clock is chip-wide. So its entries in a report carry the clock each run
saw, and split a tenant's ratio into the part the clock explains and the
part it does not. Its oracle, mfma_checksum(), is here too, in integers only.
The kind has a form (MFMA_FORMS): the bf16 instruction by default, or its fp8
twin, or the block-scaled MXFP8 and MXFP4 ones that inference tenants run,
2 x and 4 x the bf16 work per clock through the same pipe. And its operands
come from one of two places (MFMA_OPERANDS): "registers", where they stay
for the whole launch, or "lds", re-read from the workgroup's LDS before every
step as a GEMM re-reads its own, the slot rotating with the step. The LDS is
a CU's, so a mask isolates it fully; the clock it helps to pull down is not.

Concurrency comes from processes only: each child has one stream, and no
child is ever started after one has failed.

Child side: python -m elastic_gpu_scheduler_amd.agent.cotenancy --child ...
"""
from __future__ import annotations

import argparse
import functools
import json
import math
import os
import queue
import statistics
import subprocess
import sys
import threading
import time
from pathlib import Path
from typing import Any, Callable, Dict, List, Mapping, Optional, Sequence, Tuple

from elastic_gpu_scheduler_amd.agent.cumask import mask_hex
from elastic_gpu_scheduler_amd.agent.wiring import ENV_CU_MASK

KINDS = ("fma", "stream", "cache", "chase")
ALL_PAIRS: Tuple[Tuple[str, str], ...] = (
    ("fma", "fma"), ("stream", "stream"), ("fma", "stream"), ("stream", "fma"))
# The pairs that say what a neighbour does to a tenant living in a cache.
CACHE_PAIRS: Tuple[Tuple[str, str], ...] = (
    ("cache", "cache"), ("cache", "stream"), ("stream", "cache"), ("cache", "fma"))
# The pairs that say what a neighbour does to a tenant bound by latency.
CHASE_PAIRS: Tuple[Tuple[str, str], ...] = (
    ("chase", "chase"), ("chase", "stream"), ("stream", "chase"), ("chase", "fma"))
# The kind that runs on the matrix cores, and every kind there is.
MATRIX_KINDS = ("mfma",)
ALL_KINDS = KINDS + MATRIX_KINDS
# The pairs that say what a neighbour does to a tenant issuing MFMAs.
MFMA_PAIRS: Tuple[Tuple[str, str], ...] = (
    ("mfma", "mfma"), ("mfma", "stream"), ("stream", "mfma"), ("mfma", "fma"))
# What may differ from tenant to tenant, or from kind to kind, within one call.
WINDOW_KEYS = ("iters", "bytes", "passes")
# Kinds whose result carries a checksum of the buffer they read.
READING_KINDS = ("stream", "cache")

# A launch counts as contended when at least this much of it lies inside the
# other tenant's launches: the few microseconds between two back-to-back
# launches of the neighbour must not disqualify it.
CONTENDED_FRACTION = 0.95
# Never compute a ratio from fewer contended launches than this.
MIN_CONTENDED = 3
MAX_LAUNCHES = 64  # the probe's own cap
MAX_CACHE_PASSES = 65535  # the probe's own cap for the cache kind
# What a default stream launch reads (1 GiB x 127 passes). A cache launch that
# reads as much lasts about as long as a stream or fma launch beside it, so
# the balanced launch counts stay below MAX_LAUNCHES.
PAIR_LAUNCH_BYTES = 127 << 30
# What a launch of the working-set sweep reads: a few milliseconds at any size.
PROFILE_LAUNCH_BYTES = 16 << 30
CHILD_MODULE = "elastic_gpu_scheduler_amd.agent.cotenancy"

Launches = Sequence[Mapping[str, Any]]


# --- overlap ----------------------------------------------------------------

def _union(launches: Launches) -> List[Tuple[int, int]]:
    """The launches' [t0, t1] intervals, sorted and merged."""
    merged: List[Tuple[int, int]] = []
    for t0, t1 in sorted((int(l["t0"]), int(l["t1"])) for l in launches):
        if t1 <= t0:
            continue
        if merged and t0 <= merged[-1][1]:
            merged[-1] = (merged[-1][0], max(merged[-1][1], t1))
        else:
            merged.append((t0, t1))
    return merged


def overlap(launches_a: Launches, launches_b: Launches) -> List[Dict[str, Any]]:
    """For each launch of A: {"fraction", "label"}. fraction is the part of
    [t0, t1] covered by the union of B's launch intervals; label is
    "contended" (fraction >= 0.95), "solo" (nothing covered) or "mixed"
    (anything else, an empty interval included). Mixed launches count for
    no rate."""
    other = _union(launches_b)
    out = []
    for l in launches_a:
        t0, t1 = int(l["t0"]), int(l["t1"])
        if t1 <= t0:
            out.append({"fraction": 0.0, "label": "mixed"})
            continue
        covered = sum(max(0, min(t1, b1) - max(t0, b0)) for b0, b1 in other)
        fraction = covered / (t1 - t0)
        label = ("contended" if fraction >= CONTENDED_FRACTION
                 else "solo" if covered == 0 else "mixed")
        out.append({"fraction": fraction, "label": label})
    return out


def cache_passes(nbytes: int, launch_bytes: int = PAIR_LAUNCH_BYTES) -> int:
    """The odd number of passes with which a cache tenant of `nbytes` reads
    about `launch_bytes` per launch, within the probe's 1..65535."""
    return min(MAX_CACHE_PASSES, max(1, launch_bytes // max(int(nbytes), 16))) | 1


# --- the chase tenant's oracle ------------------------------------------------

def chase_stride(nodes: int) -> int:
    """The chase tenant's hop: next(i) = (i + stride) % nodes. The first of
    s0, s0 + 1, ... coprime to `nodes`, from s0 = nodes * 28657 // 46368 (a
    Fibonacci ratio, about 0.618), so the chain is one cycle through every
    node; 0 for a single node, which loops on itself."""
    nodes = int(nodes)
    if nodes < 1:
        raise ValueError("a chase buffer has at least one node")
    stride = nodes * 28657 // 46368
    while math.gcd(stride, nodes) != 1:
        stride += 1
    return stride


def chase_checksum(nbytes: int, workgroups: int, iters: int, seed: int) -> int:
    """What a chase tenant's checksum must be: the buffer of `nbytes` (a
    multiple of 128) is nbytes // 128 nodes; wave w of the 4 * `workgroups`
    starts at (seed + w * nodes // W) % nodes and ends `iters` hops of
    chase_stride(nodes) further on; each of its 64 lanes g = 64 w .. 64 w +
    63 adds (g + 1) * (end + 1), modulo 2^64."""
    nodes = int(nbytes) // 128
    stride, waves = chase_stride(nodes), 4 * int(workgroups)
    total = 0
    for w in range(waves):
        end = (seed + w * nodes // waves + iters * stride) % nodes
        # the sum of g + 1 over the wave's lanes
        total += (64 * 64 * w + 64 * 65 // 2) * (end + 1)
    return total % (1 << 64)


# --- the mfma tenant's oracle -------------------------------------------------

MFMA_VARIANTS = 16  # operand sets; wave w uses w % 16
# The instruction an mfma tenant issues: "bf16" v_mfma_f32_32x32x16_bf16,
# "fp8" its e4m3 twin, "mxfp8" and "mxfp4" the block-scaled 32x32x64 with e4m3
# and e2m1 operands. Position is the form's id in the probe.
MFMA_FORMS = ("bf16", "fp8", "mxfp8", "mxfp4")
# Per form, as in csrc/gpuprobe/cotenant.hip: the K of one MFMA, its flop,
# the steps between two folds and the steps of a default launch.
MFMA_FORM_TABLE: Dict[str, Dict[str, int]] = {
    "bf16": {"k": 16, "flop": 32768, "chunk": 2048, "iters": 32768},
    "fp8": {"k": 16, "flop": 32768, "chunk": 2048, "iters": 32768},
    "mxfp8": {"k": 64, "flop": 131072, "chunk": 512, "iters": 16384},
    "mxfp4": {"k": 64, "flop": 131072, "chunk": 256, "iters": 32768},
}
# Where an mfma tenant's operands come from: kept in registers for the whole
# launch, or re-read from LDS before every step.
MFMA_OPERANDS = ("registers", "lds")
# Operands from LDS, as in csrc/gpuprobe/cotenant.hip: a workgroup's image is
# one slot per wave, and a slot is the bytes a wave reads per step.
MFMA_LDS_SLOTS = 4
MFMA_LDS_STEP_BYTES: Dict[str, int] = {
    "bf16": 4096, "fp8": 2048, "mxfp8": 9216, "mxfp4": 5120}
# Twice the magnitude of e2m1 code & 7 (0, 0.5, 1, 1.5, 2, 3, 4, 6): the mxfp4
# scales are 2 or 4, so every effective element is an integer.
_E2M1_TWICE = (0, 1, 2, 3, 4, 6, 8, 12)
_M32 = 0xFFFFFFFF


def _mix32(x: int) -> int:
    x &= _M32
    x ^= x >> 16
    x = x * 0x7FEB352D & _M32
    x ^= x >> 15
    x = x * 0x846CA68B & _M32
    x ^= x >> 16
    return x


def _mfma_elem(form: int, h: int, scale_bit: int, is_a: bool) -> int:
    """The effective integer a hashed element stands for in form id `form`:
    bf16 and fp8 h % 31 - 15; mxfp8 (h % 15 - 7) * 2^e; mxfp4 the e2m1 code
    h & 15 times its block scale, 2^(1 + e) for A and 2 for B."""
    if form < 2:
        return h % 31 - 15
    if form == 2:
        return (h % 15 - 7) << scale_bit
    mag = _E2M1_TWICE[h & 7] << (scale_bit if is_a else 0)
    return -mag if h & 8 else mag


def _mfma_a(key: int, row: int, k: int, form: int = 0) -> int:
    """A[row][k] of one operand variant, scale applied: bf16 and fp8 -15..15,
    mxfp8 -14..14, mxfp4 -24..24."""
    f = form << 24
    h = _mix32(key ^ (row << 8) ^ k ^ 0x00A00000 ^ f)
    e = _mix32(key ^ (row << 8) ^ (k // 32) ^ 0x00E00000 ^ f) & 1 if form >= 2 else 0
    return _mfma_elem(form, h, e, True)


def _mfma_b(key: int, k: int, col: int, form: int = 0) -> int:
    """B[k][col] of one operand variant, scale applied: bf16 and fp8 -15..15,
    mxfp8 -14..14, mxfp4 -12..12."""
    f = form << 24
    h = _mix32(key ^ (k << 8) ^ col ^ 0x00B00000 ^ f)
    e = _mix32(key ^ ((k // 32) << 8) ^ col ^ 0x00F00000 ^ f) & 1 if form == 2 else 0
    return _mfma_elem(form, h, e, False)


def _mfma_product(seed: int, variant: int, form: int = 0) -> List[List[int]]:
    """The 64 x 64 product one step adds to a wave's tile: A (64 x K) times
    B (K x 64) of `variant`, hashed from the low 32 bits of `seed`; K is the
    form's. The probe lays A and B into the lanes by one rule, and every
    element under the scale of its own block of 32 k, so which lane holds
    which k does not enter the product."""
    depth = MFMA_FORM_TABLE[MFMA_FORMS[form]]["k"]
    key = _mix32((seed & _M32) ^ (variant * 0x9E3779B1 & _M32))
    a = [[_mfma_a(key, row, k, form) for k in range(depth)] for row in range(64)]
    cols = [[_mfma_b(key, k, col, form) for k in range(depth)] for col in range(64)]
    return [[sum(x * y for x, y in zip(a[row], cols[col])) for col in range(64)]
            for row in range(64)]


@functools.lru_cache(maxsize=16)
def _mfma_lane_sums(seed32: int, form: int = 0) -> Tuple[Tuple[int, ...], ...]:
    """Per variant and lane, what one step adds to the lane's fold: lane r =
    lane & 31, h = lane >> 5 holds, in register reg of accumulator (m, n),
    row 32 m + (reg & 3) + 8 (reg >> 2) + 4 h of column 32 n + r, and weighs
    it by 1 + reg + 16 (2 m + n). The same for every form."""
    out = []
    for variant in range(MFMA_VARIANTS):
        p = _mfma_product(seed32, variant, form)
        lanes = []
        for lane in range(64):
            r, h = lane & 31, lane >> 5
            lanes.append(sum(
                p[32 * m + (reg & 3) + 8 * (reg >> 2) + 4 * h][32 * n + r]
                * (1 + reg + 16 * (2 * m + n))
                for m in range(2) for n in range(2) for reg in range(16)))
        out.append(tuple(lanes))
    return tuple(out)


# What an mfma tenant may be told beyond its window, in the order its child
# is told, each with the values it may take.
_MFMA_OPTIONS = {"form": MFMA_FORMS, "operands": MFMA_OPERANDS}


def _checked(key: str, value: Optional[str]) -> str:
    if value not in _MFMA_OPTIONS[key]:
        raise ValueError(f"unknown mfma {key} {value!r}: one of "
                         + ", ".join(_MFMA_OPTIONS[key]))
    return value


def _mfma_option(key: str, tenant: Mapping[str, Any], kind: str,
                 wide: Optional[str]) -> Optional[str]:
    """The option `key` that `tenant`, run as `kind`, is started with: its
    own, else the call-wide `wide`; None when neither names one."""
    own = tenant.get(key)
    if kind not in MATRIX_KINDS:
        if own is not None:
            raise ValueError(f"a {kind} tenant takes no {key}: {own!r}")
        return None
    value = wide if own is None else own
    return value if value is None else _checked(key, value)


def mfma_checksum(workgroups: int, iters: int, seed: int, form: str = "bf16",
                  operands: str = "registers") -> int:
    """What an mfma tenant's checksum must be. Wave w of the 4 * `workgroups`
    multiplies variant w % 16 of the operands, small integers hashed from the
    low 32 bits of `seed`, `iters` times into its 64 x 64 tile, and every
    lane folds its 64 accumulator registers, weighted, into one sum. The
    accumulators are exact and every fold is linear in the number of steps,
    so a lane's sum is iters times what one step adds; lane g = 64 w + lane
    adds (g + 1) times its sum, modulo 2^64.

    `form` is one of MFMA_FORMS (anything else raises ValueError). The forms
    differ in the operands only: the hash takes the form's id, "fp8" holds
    the same -15..15 as e4m3, "mxfp8" -7..7 as e4m3 and "mxfp4" e2m1 codes,
    both at K = 64 under a scale of 2^e per row or column and block of 32 k
    (mxfp8: e in {0, 1} on both sides; mxfp4: 1 + e for A, 1 for B), so that
    every effective element is an integer and the product is taken from
    integer matrices as for bf16.

    `operands` is one of MFMA_OPERANDS (anything else raises ValueError).
    With "lds" the four waves of a workgroup share the four variants they
    built: at step i of the launch wave w multiplies the fragments of slot
    (w + i) & 3, that is variant v_s = (w & ~3) % 16 + ((w + s) & 3) at the
    n_s = iters // 4 + (1 if s < iters % 4 else 0) steps with i % 4 = s, so
    its lane folds to the sum over s = 0..3 of n_s times what one step of
    v_s adds. With one step that is the wave's own variant, as from
    registers."""
    sums = _mfma_lane_sums(int(seed) & _M32, MFMA_FORMS.index(_checked("form", form)))
    waves = 4 * int(workgroups)
    total = 0
    if _checked("operands", operands) == "lds":
        steps = [int(iters) // 4 + (1 if s < int(iters) % 4 else 0) for s in range(4)]
        for first in range(min(MFMA_VARIANTS, waves)):  # the waves w % 16 == first
            mine = range(first, waves, MFMA_VARIANTS)
            lanes = [sum(n * sums[(first & ~3) + ((first + s) & 3)][lane]
                         for s, n in enumerate(steps)) for lane in range(64)]
            total += 64 * sum(mine) * sum(lanes) + len(mine) * sum(
                (lane + 1) * s for lane, s in enumerate(lanes))
        return total % (1 << 64)
    for variant, lanes in enumerate(sums):
        mine = range(variant, waves, MFMA_VARIANTS)  # the waves of this variant
        # the sum over them of (64 w + lane + 1) * lanes[lane]
        total += 64 * sum(mine) * sum(lanes) + len(mine) * sum(
            (lane + 1) * s for lane, s in enumerate(lanes))
    return total * int(iters) % (1 << 64)


# --- child ------------------------------------------------------------------

def _child_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="cotenancy", description=__doc__)
    p.add_argument("--child", action="store_true", required=True)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--kind", choices=ALL_KINDS, default="fma")
    p.add_argument("--launches", type=int, default=8)
    p.add_argument("--iters", type=int, default=0)
    p.add_argument("--bytes", type=int, default=0)
    p.add_argument("--passes", type=int, default=0)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--form", choices=MFMA_FORMS, default="bf16")
    p.add_argument("--operands", choices=MFMA_OPERANDS, default=None)
    return p


def child_main(argv: Optional[Sequence[str]] = None, stdin=None, stdout=None) -> int:
    """One tenant: warm up, say READY, wait for GO, run, print TENANT <json>.
    The CU mask is whatever ROC_GLOBAL_CU_MASK this process was started
    under, so the probe is given a plain stream."""
    args = _child_parser().parse_args(argv)
    stdin = sys.stdin if stdin is None else stdin
    stdout = sys.stdout if stdout is None else stdout
    from elastic_gpu_scheduler_amd._native import gpuprobe

    probe = gpuprobe()
    window = {"kind": args.kind, "iters": args.iters, "bytes": args.bytes,
              "passes": args.passes, "seed": args.seed}
    # The form is the mfma kind's; beside another kind only a form the probe
    # would refuse is handed on, so that it does refuse it.
    if args.kind in MATRIX_KINDS or args.form != MFMA_FORMS[0]:
        window["form"] = args.form
    # Likewise the operands, and only when named: the probe refuses "lds"
    # beside another kind.
    if args.operands is not None:
        window["operands"] = args.operands
    warm = probe.cu_tenant_run(args.device, None, launches=1, **window)
    if "skipped" in warm:
        print(f"cotenancy child: {warm}", file=sys.stderr)
        return 4
    print("READY", file=stdout, flush=True)
    if stdin.readline().strip() != "GO":
        return 3
    result = probe.cu_tenant_run(args.device, None, launches=args.launches, **window)
    print("TENANT " + json.dumps(result), file=stdout, flush=True)
    return 0


# --- parent -----------------------------------------------------------------

def _spawn(argv: List[str], env: Dict[str, str]):
    """A fresh process, never exec: the parent may hold the GPU."""
    return subprocess.Popen(argv, env=env, stdin=subprocess.PIPE,
                            stdout=subprocess.PIPE, text=True)


class _Trouble(Exception):
    pass


class _Child:
    """One started tenant: its output lines arrive through a reader thread,
    so that every wait on it ends at the child's own deadline."""

    def __init__(self, index: int, proc, timeout: float) -> None:
        self.index = index
        self.proc = proc
        self.deadline = time.monotonic() + timeout
        self.lines: "queue.Queue[Optional[str]]" = queue.Queue()
        threading.Thread(target=self._pump, daemon=True).start()

    def _pump(self) -> None:
        try:
            for line in self.proc.stdout:
                self.lines.put(line)
        finally:
            self.lines.put(None)

    def _fail(self, what: str) -> _Trouble:
        return _Trouble({"tenant": self.index, "what": what,
                         "returncode": self.proc.poll()})

    def expect(self, prefix: str) -> str:
        while True:
            left = self.deadline - time.monotonic()
            try:
                if left <= 0:
                    raise queue.Empty
                line = self.lines.get(timeout=left)
            except queue.Empty:
                raise self._fail(f"timed out waiting for {prefix}") from None
            if line is None:
                try:  # the exit status belongs in the detail
                    self.proc.wait(timeout=max(self.deadline - time.monotonic(), 0.1))
                except subprocess.TimeoutExpired:
                    pass
                raise self._fail(f"no {prefix} line")
            if line.startswith(prefix):
                return line[len(prefix):].strip()

    def go(self) -> None:
        try:
            self.proc.stdin.write("GO\n")
            self.proc.stdin.flush()
        except (OSError, ValueError):
            raise self._fail("could not be told GO") from None

    def finish(self) -> None:
        try:
            code = self.proc.wait(timeout=max(self.deadline - time.monotonic(), 0.1))
        except subprocess.TimeoutExpired:
            raise self._fail("timed out before exiting") from None
        if code != 0:
            raise self._fail(f"exit status {code}")

    def kill(self) -> None:
        if self.proc.poll() is None:
            self.proc.kill()
            try:
                self.proc.wait(timeout=10)
            except subprocess.TimeoutExpired:
                pass


def run_pair(card: int, tenants: Sequence[Mapping[str, Any]],
             kinds: Optional[Sequence[str]] = None, *, launches: int = 8,
             iters: int = 0, bytes: int = 0, passes: int = 0, seed: int = 1,
             timeout: float = 120.0,
             spawn: Optional[Callable[[List[str], Dict[str, str]], Any]] = None,
             form: Optional[str] = None,
             operands: Optional[str] = None) -> Dict[str, Any]:
    """Run up to two tenants at once on `card`, each a fresh child process
    under ROC_GLOBAL_CU_MASK = its mask. A tenant is {"mask": int, "kind":
    "fma" | "stream" | "cache" | "chase" | "mfma"} and may carry its own "launches", "iters",
    "bytes" and "passes" in place of the call-wide ones; `kinds`, when given,
    names the kinds instead. Every child warms up and says READY; only then
    are all told GO. Returns {"ok": True, "tenants": [the children's
    cu_tenant_run results]}.

    `form` (one of MFMA_FORMS) is the instruction of every mfma tenant of
    the call and leaves the others as they are; an mfma tenant may carry its
    own "form" instead. An unknown form, or a "form" on a tenant of another
    kind, raises ValueError before anything is started. A child is given
    --form only when a form was named for it.

    `operands` (one of MFMA_OPERANDS) says where every mfma tenant of the
    call takes its operands from, by the same rules: an mfma tenant may
    carry its own "operands" instead, an unknown value or "operands" on a
    tenant of another kind raises ValueError before anything is started,
    and a child is given --operands, after --form, only when one was named
    for it.

    Each child has `timeout` seconds from its start. The first child that
    times out, exits non-zero or prints no TENANT line ends the run: the
    others are killed and {"ok": False, "reason": "child-failed", "detail"}
    is returned. Nothing is retried."""
    if not 1 <= len(tenants) <= 2:
        raise ValueError("run_pair takes one or two tenants")
    if kinds is not None and len(kinds) != len(tenants):
        raise ValueError("one kind per tenant")
    call = {"form": form, "operands": operands}
    for key, value in call.items():
        if value is not None:
            _checked(key, value)
    # Per tenant, what its child is told of each option; None: nothing.
    options: List[Dict[str, Optional[str]]] = []
    for i, tenant in enumerate(tenants):
        kind = kinds[i] if kinds is not None else tenant["kind"]
        options.append({key: _mfma_option(key, tenant, kind, wide)
                        for key, wide in call.items()})
    spawn = _spawn if spawn is None else spawn
    root = str(Path(__file__).resolve().parents[2])
    children: List[_Child] = []
    try:
        for i, tenant in enumerate(tenants):
            kind = kinds[i] if kinds is not None else tenant["kind"]
            if kind not in ALL_KINDS:
                raise ValueError(f"unknown tenant kind {kind!r}")
            env = dict(os.environ)
            env[ENV_CU_MASK] = mask_hex(int(tenant["mask"]))
            env["PYTHONPATH"] = os.pathsep.join(
                [root] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
            argv = [sys.executable, "-m", CHILD_MODULE, "--child",
                    "--device", str(card), "--kind", kind,
                    "--launches", str(int(tenant.get("launches", launches))),
                    "--iters", str(tenant.get("iters", iters)),
                    "--bytes", str(tenant.get("bytes", bytes)),
                    "--passes", str(tenant.get("passes", passes)),
                    "--seed", str(seed)]
            for key, value in options[i].items():
                if value is not None:
                    argv += ["--" + key, value]
            try:
                proc = spawn(argv, env)
            except OSError as exc:
                raise _Trouble({"tenant": i, "what": f"not started: {exc}",
                                "returncode": None}) from None
            children.append(_Child(i, proc, timeout))
        results: List[Optional[Dict[str, Any]]] = [None] * len(children)
        for c in children:
            c.expect("READY")
        for c in children:
            c.go()
        for c in children:
            results[c.index] = json.loads(c.expect("TENANT "))
            c.finish()
        return {"ok": True, "tenants": results}
    except _Trouble as trouble:
        return {"ok": False, "reason": "child-failed", "detail": trouble.args[0]}
    finally:
        for c in children:
            c.kill()


def _pattern_checksum(seed: int, nbytes: int) -> int:
    """XOR of the pattern over a buffer of `nbytes`: the probe's host oracle,
    which takes at most 2^28 words at a time."""
    from elastic_gpu_scheduler_amd._native import gpuprobe

    probe = gpuprobe()
    words, first, x = nbytes // 8, 0, 0
    while first < words:
        n = min(words - first, 1 << 28)
        x ^= probe.pattern_xor(seed, first, n)
        first += n
    return x


def _balanced(launches: int, seconds: Sequence[float]) -> List[int]:
    """Launch counts that make both tenants run about equally long. The
    work of a launch is left as it was measured solo; the tenant whose
    launches are more than a quarter shorter gets more of them, twice what
    the solo durations ask for because contention may slow either side, up
    to the probe's cap. What it runs past the neighbour's end is labelled
    solo and dropped."""
    longest = max(seconds)
    out = []
    for s in seconds:
        if s <= 0 or longest / s <= 1.25:
            out.append(launches)
        else:
            out.append(min(MAX_LAUNCHES, math.ceil(2.0 * launches * longest / s) + 1))
    return out


# What a report knows of each kind. First the keys of a child's result that a
# solo entry adds; a kind that adds clock_ghz gets the clock split in a pair.
_SOLO_KEYS = {"chase": ("ns_per_hop",), "mfma": ("clock_ghz",)}


def _expected(result: Mapping[str, Any], seed: int, pattern, form=None,
              operands=None) -> Optional[int]:
    """The checksum a child's result must carry by the oracle of its kind
    (`pattern` is the reading kinds'); None for a kind that has none."""
    kind = result["kind"]
    if kind in READING_KINDS:
        return pattern(seed, int(result["bytes"]))
    if kind == "chase":
        return chase_checksum(result["bytes"], result["workgroups"], result["iters"], seed)
    if kind in MATRIX_KINDS:
        return mfma_checksum(result["workgroups"], result["iters"], seed,
                             form or MFMA_FORMS[0], operands or MFMA_OPERANDS[0])
    return None


def isolation_report(card: int, tenants: Sequence[Mapping[str, Any]], *,
                     pairs: Sequence[Tuple[str, str]] = ALL_PAIRS,
                     launches: int = 8, iters: int = 0, bytes: int = 0,
                     passes: int = 0, seed: int = 1, timeout: float = 120.0,
                     spawn: Optional[Callable[..., Any]] = None,
                     expected_checksum: Optional[Callable[[int, int], int]] = None,
                     windows: Optional[Mapping[str, Mapping[str, int]]] = None,
                     form: Optional[str] = None,
                     operands: Optional[str] = None) -> Dict[str, Any]:
    """Each of two tenants' ({"mask": int}) rate alone and next to the other.

    First one solo run per tenant and kind that `pairs` uses, then the pairs
    in the order given (default fma/fma, stream/stream, fma/stream,
    stream/fma; the first kind is tenant 0's). Returns {"ok", "solo": [per
    tenant {kind: {rate, seconds, launches, workgroups}}], "pairs": {"a/b": {"ok",
    "tenants": [{kind, solo_rate, contended_rate, ratio, contended_launches,
    launches}]}}}. contended_rate is the median over the launches that lay
    inside the other tenant's launches (overlap()); with fewer than three of
    them the tenant gets reason "no-overlap" and no ratio.

    `windows` gives a kind its own iters / bytes / passes in place of the
    call-wide ones, in the solo runs and in the pairs alike, for example
    {"cache": {"bytes": 12 << 20, "passes": cache_passes(12 << 20)},
    "stream": {"bytes": 1 << 30}}: a small cache tenant next to a large
    streamer. A cache launch at the probe's default passes lasts about a
    millisecond, a default stream launch over twenty: give the cache kind
    cache_passes(bytes), or the launch count it would need to keep up is cut
    at 64 and the neighbour's launches past its end are dropped as solo.

    A chase tenant (pairs=CHASE_PAIRS) takes `bytes` and `iters`, hops per
    wave and launch; its rates are Ghop/s, its solo entry adds ns_per_hop,
    and its checksum is held against chase_checksum(), not against
    `expected_checksum`, which stays the oracle of the reading kinds.

    An mfma tenant (pairs=MFMA_PAIRS) takes `iters`, steps of four MFMAs per
    wave and launch; its rates are GFLOP/s and its checksum is held against
    mfma_checksum(). Its solo entry adds clock_ghz, the shader clock it ran
    at, and its entry in a pair adds solo_clock_ghz, contended_clock_ghz
    (the median over the contended launches), clock_ratio = contended clock
    / solo clock and cycle_ratio = ratio / clock_ratio. The chip lowers its
    clock under matrix load for the whole chip, whatever the masks, so
    clock_ratio is the part of a slowdown that the clock explains and
    cycle_ratio the part that it does not: a tenant slowed only by the
    neighbour's effect on the clock has cycle_ratio 1.

    `form` (one of MFMA_FORMS, anything else raises ValueError) is the
    instruction the mfma tenants issue, alone and in every pair; a tenant
    ({"mask": int, "form": str}) may name its own instead, for a bf16 tenant
    beside an mxfp4 one. The other kinds are not touched by it. A tenant's
    checksum is held against mfma_checksum() of its own form, and its mfma
    entries, solo and in a pair, add "form". With no form named anywhere the
    children are started as before, run bf16, and no entry has "form".

    `operands` (one of MFMA_OPERANDS, anything else raises ValueError) says
    where the mfma tenants take their operands from, alone and in every
    pair: "registers", or "lds" for tenants that re-read them from LDS
    before every step; a tenant ({"mask": int, "operands": str}) may name
    its own instead. The other kinds are not touched by it. A tenant's
    checksum is held against mfma_checksum() of its own form and operands,
    and its mfma entries, solo and in a pair, add "operands". With none
    named anywhere the children are started as before, keep their operands
    in registers, and no entry has "operands".

    ok says that the measurement is valid (every child exited 0, every
    stream and cache checksum equals the pattern's, every chase and mfma
    checksum the closed form's, overlap was reached), not that the
    tenants are isolated: no interference threshold is built in, on ratio,
    clock_ratio or cycle_ratio. The first
    child that fails ends the report ("child-failed"): nothing further is
    started."""
    if len(tenants) != 2:
        raise ValueError("isolation_report takes two tenants")
    for pair in pairs:
        if len(pair) != 2 or any(k not in ALL_KINDS for k in pair):
            raise ValueError(f"not a pair of tenant kinds: {pair!r}")
    windows = {kind: dict(w) for kind, w in (windows or {}).items()}
    for kind, w in windows.items():
        if kind not in ALL_KINDS or any(k not in WINDOW_KEYS for k in w):
            raise ValueError(f"not a window of a tenant kind: {kind!r}: {w!r}")
    # Per option and tenant, what the tenant is started with as an mfma one.
    named = {key: [_mfma_option(key, t, MATRIX_KINDS[0], wide) for t in tenants]
             for key, wide in (("form", form), ("operands", operands))}
    # The pattern's oracle, asked once per size.
    pattern = functools.lru_cache(maxsize=None)(expected_checksum or _pattern_checksum)
    window = {"iters": iters, "bytes": bytes, "passes": passes, "seed": seed,
              "timeout": timeout, "spawn": spawn}
    report: Dict[str, Any] = {"ok": True, "solo": [{}, {}], "pairs": {}}

    def flaw(reason: str, **more: Any) -> None:
        report["ok"] = False
        report.setdefault("reason", reason)
        for k, v in more.items():
            report.setdefault(k, v)

    def options(i: int, kind: str) -> Dict[str, str]:
        """The options named for tenant i, if `kind` takes any."""
        found = {key: _mfma_option(key, {}, kind, own[i]) for key, own in named.items()}
        return {key: value for key, value in found.items() if value is not None}

    def asked(i: int, kind: str) -> Dict[str, Any]:
        """What tenant i is started with as `kind`, beyond mask and launches."""
        return {**windows.get(kind, {}), **options(i, kind)}

    def sound(result: Mapping[str, Any], i: int) -> Optional[str]:
        """Why the result of tenant i's child cannot be used, or None."""
        if "skipped" in result:
            return "insufficient-memory"
        expected = _expected(result, seed, pattern, **options(i, result["kind"]))
        if expected is not None and int(result["checksum"]) != expected:
            return "bad-checksum"
        return None

    for i, tenant in enumerate(tenants):
        for kind in ALL_KINDS:
            if not any(pair[i] == kind for pair in pairs):
                continue
            run = run_pair(card, [{"mask": tenant["mask"], "kind": kind,
                                   **asked(i, kind)}],
                           launches=launches, **window)
            if not run["ok"]:
                flaw(run["reason"], detail=run["detail"])
                return report
            result = run["tenants"][0]
            why = sound(result, i)
            if why == "insufficient-memory":
                flaw(why)
                return report
            if why:
                flaw(why)
            report["solo"][i][kind] = {
                "rate": result["rate"],
                "seconds": statistics.median(l["seconds"] for l in result["launches"]),
                "launches": len(result["launches"]),
                "workgroups": result.get("workgroups"),
                **{key: result[key] for key in _SOLO_KEYS.get(kind, ())},
                **options(i, kind)}

    for pair in pairs:
        name = "/".join(pair)
        counts = _balanced(launches, [report["solo"][i][pair[i]]["seconds"]
                                      for i in range(2)])
        run = run_pair(card, [{"mask": tenants[i]["mask"], "kind": pair[i],
                               "launches": counts[i], **asked(i, pair[i])}
                              for i in range(2)],
                       launches=launches, **window)
        if not run["ok"]:
            flaw(run["reason"], detail=run["detail"])
            report["pairs"][name] = {"ok": False, "reason": run["reason"]}
            return report
        results = run["tenants"]
        entry: Dict[str, Any] = {"ok": True, "tenants": []}
        for i in range(2):
            why = sound(results[i], i)
            if why == "insufficient-memory":
                flaw(why)
                report["pairs"][name] = {"ok": False, "reason": why}
                return report
            mine, other = results[i]["launches"], results[1 - i]["launches"]
            labels = [o["label"] for o in overlap(mine, other)]
            rates = [l["rate"] for l, lab in zip(mine, labels) if lab == "contended"]
            solo_rate = report["solo"][i][pair[i]]["rate"]
            t: Dict[str, Any] = {
                "kind": pair[i], "solo_rate": solo_rate,
                "contended_launches": len(rates), "launches": len(mine),
                "solo_launches": labels.count("solo"),
                "mixed_launches": labels.count("mixed"),
                **options(i, pair[i])}
            if len(rates) < MIN_CONTENDED:
                why = why or "no-overlap"
            else:
                t["contended_rate"] = statistics.median(rates)
                t["ratio"] = t["contended_rate"] / solo_rate
                if "clock_ghz" in _SOLO_KEYS.get(pair[i], ()):
                    clocks = [l["clock_ghz"] for l, lab in zip(mine, labels)
                              if lab == "contended"]
                    t["solo_clock_ghz"] = report["solo"][i][pair[i]]["clock_ghz"]
                    t["contended_clock_ghz"] = statistics.median(clocks)
                    t["clock_ratio"] = t["contended_clock_ghz"] / t["solo_clock_ghz"]
                    t["cycle_ratio"] = t["ratio"] / t["clock_ratio"]
            if why:
                t["reason"] = why
                entry["ok"] = False
                entry.setdefault("reason", why)
                flaw(why)
            entry["tenants"].append(t)
        report["pairs"][name] = entry
    return report


def _profile(card: int, mask: int, kind: str, sizes: Sequence[int], window: Callable,
             row: Callable, pattern: Optional[Callable], seed: int, **how: Any):
    """The loop of cache_profile and chase_profile: one child per size, given
    `bytes` = the size and window(size); a row is row(its result, the median
    of its launches' seconds)."""
    out: Dict[str, Any] = {"ok": True, "profile": []}
    for size in sizes:
        size = int(size)
        run = run_pair(card, [{"mask": mask, "kind": kind, "bytes": size,
                               **window(size)}], seed=seed, **how)
        if not run["ok"]:
            out.update(ok=False, reason=run["reason"], detail=run["detail"])
            return out
        result = run["tenants"][0]
        if "skipped" in result:
            out.update(ok=False, reason="insufficient-memory")
            return out
        if int(result["checksum"]) != _expected(result, seed, pattern):
            out["ok"] = False
            out.setdefault("reason", "bad-checksum")
        out["profile"].append(row(result, statistics.median(
            l["seconds"] for l in result["launches"])))
    return out


def cache_profile(card: int, mask: int, sizes: Sequence[int], *,
                  launches: int = 8, passes: int = 0, seed: int = 1,
                  timeout: float = 120.0,
                  spawn: Optional[Callable[..., Any]] = None,
                  expected_checksum: Optional[Callable[[int, int], int]] = None
                  ) -> Dict[str, Any]:
    """One cache tenant alone under `mask`, once per working-set size: where
    the rate steps down is where the working set stops fitting a cache. One
    child per size, in the order given, never two at once. `passes` 0 reads
    about 16 GiB per launch at every size (cache_passes). Returns {"ok",
    "profile": [{bytes, bytes_per_cu, rate, seconds, passes}]}, rate in GB/s
    and seconds the median over the launches.

    The first child that fails ends the sweep ("child-failed"), as does one
    that finds too little free memory; a wrong checksum makes it not ok but
    the figures are kept. Nothing is retried."""
    return _profile(
        card, mask, "cache", sizes,
        lambda size: {"passes": passes or cache_passes(size, PROFILE_LAUNCH_BYTES)},
        lambda result, seconds: {
            "bytes": result["bytes"], "bytes_per_cu": result.get("bytes_per_cu"),
            "rate": result["rate"], "seconds": seconds, "passes": result["passes"]},
        expected_checksum or _pattern_checksum, seed,
        launches=launches, timeout=timeout, spawn=spawn)


def chase_profile(card: int, mask: int, sizes: Sequence[int], *,
                  launches: int = 8, iters: int = 0, seed: int = 1,
                  timeout: float = 120.0,
                  spawn: Optional[Callable[..., Any]] = None) -> Dict[str, Any]:
    """One chase tenant alone under `mask`, once per working-set size: where
    the time per hop steps up is where the working set stops fitting a cache,
    and each plateau is that level's dependent-load latency with one load in
    flight per wave. One child per size, in the order given, never two at
    once. `iters` 0 is the probe's default, 65536 hops per wave and launch.
    Returns {"ok", "profile": [{bytes, nodes, iters, ns_per_hop, rate,
    seconds}]}, rate in Ghop/s, ns_per_hop and seconds the median over the
    launches.

    The first child that fails ends the sweep ("child-failed"), as does one
    that finds too little free memory; a wrong checksum (chase_checksum)
    makes it not ok but the figures are kept. Nothing is retried."""
    return _profile(
        card, mask, "chase", sizes, lambda size: {"iters": iters},
        lambda result, seconds: {
            "bytes": result["bytes"], "nodes": result["nodes"],
            "iters": result["iters"], "ns_per_hop": result["ns_per_hop"],
            "rate": result["rate"], "seconds": seconds},
        None, seed, launches=launches, timeout=timeout, spawn=spawn)


if __name__ == "__main__":
    sys.exit(child_main())
