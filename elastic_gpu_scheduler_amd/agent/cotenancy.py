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

A sixth kind, "gemm" (GEMM_KINDS, EVERY_KIND, GEMM_PAIRS), is the tenant
the mfma kind was walked towards: a whole bf16 GEMM whose operands start in
device memory and travel global -> LDS -> MFMA, the one load that draws on
the memory path, the LDS and the matrix pipe in one kernel. Its window is
`bytes` (A plus B), `iters` (steps of 64 k) and `passes` (whole GEMMs per
launch); gemm_shape() states the shape they give and gemm_checksum() what
the launch must sum to, in integers and in closed form. Like mfma it
reports the clock it saw, so a pair splits its ratio the same way: beside
a streamer both the chip-wide clock and the shared memory path move, and
cycle_ratio is the part that is not the clock. It takes no form and no
operands. Its slabs reach LDS in one of two ways (GEMM_LOADS): "registers",
global_load into registers and ds_write from them, or "direct", the
16-byte LDS-DMA load of gfx950 that production GEMMs there use, a ring of
slab pairs in LDS and no register in between. The product, and so the
checksum, is the same.

Two more kinds, "gemm-mxfp8" and "gemm-mxfp4" (MXGEMM_KINDS, TENANT_KINDS,
mxgemm_pairs()), are that GEMM in the forms inference tenants run: e4m3 or
e2m1 elements under one E8M0 scale per row and block of 32 k, the elements
through LDS, the scales from memory straight to registers, two slabs in
flight. The form is part of the kind's name, so they too take neither form
nor operands; their window is the gemm kind's with a step of 128 or 256 k,
and gemm_shape() and gemm_checksum() take the form as a keyword.

Two more again, "decode-mxfp8" and "decode-mxfp4" (DECODE_KINDS, CO_KINDS,
decode_pairs()), are the other shape of the same block-scaled GEMM, the one
an inference tenant spends most of its time in: 32 token rows against a
weight matrix that is read once, C (32 x N) = A (32 x K) . W^T. Every byte
of W is used for 32 rows and never again, so HBM sets the pace and not the
matrix pipe: the one tenant that loads the matrix cores and the memory
system together. W goes from memory straight to registers in fragment
layout, several steps in flight per wave; the 32 rows of A are shared by a
workgroup's waves through LDS. Their window is `bytes` (W's elements, 0: 1
GiB, more than the Infinity Cache holds), `iters` (steps of 128 or 256 k, 0:
K = 8192) and `passes` (whole re-reads of W); decode_shape() states the
shape and gemm_checksum(32, n, k, ...) is the oracle unchanged. They take
neither form nor operands nor loads. W lies in memory in one of two ways
(DECODE_WEIGHTS): "rows", row-major, where every lane of a weight load sits
on a row of its own and one wave instruction touches 32 lines of 128 bytes
for 1 KiB, or "tiled", the 16-byte chunks stored once in the order a wave
consumes them (units of 32 rows x one step, 4 KiB), where it reads 8 whole
lines and a wave's K is one contiguous run: what production decode GEMMs on
this chip do with their weights offline. The elements, the scales, the
product and so the checksum are the same. TENANT_KINDS stays the kinds
before them; CO_KINDS is those and the decode kinds.

The last kind, "attention" (ATTENTION_KINDS, WORKLOAD_KINDS,
attention_pairs()), is the other kernel a transformer tenant spends its
prefill in: a causal flash-attention forward pass in bf16, head dimension
128. It keeps the matrix pipe and the transcendental unit (v_exp_f32) busy
in one wave, re-reads a head's K and V out of L2 and the Infinity Cache once
per query tile, and its workgroups are not equally long, so a launch has a
tail. Its window is `iters` (the sequence length in units of 128 rows, 0:
8192 rows), `bytes` (Q plus K plus V, 0: 64 heads) and `passes` (whole
forward passes per launch); attention_shape() states the shape and
attention_operands() the data. Its output is no integer, so it has no
checksum: the probe recomputes 256 sampled rows in fp64 after the timed
launches and reports max_error, which a report holds against
ATTENTION_TOLERANCE. It reports the clock it saw and a pair splits its ratio
as for the GEMM kinds; it takes neither form nor operands nor loads nor
weights. WORKLOAD_KINDS is the kinds up to here.

"attention-decode" (ATTENTION_DECODE_KINDS, SERVING_KINDS,
attention_decode_pairs()) is the other half of attention, a decode step's: the
16 query rows of one step (a grouped-query group of 16) attend to a head's K
and V, which are read from HBM exactly once per pass, the work split along the
keys, MFMA, v_exp_f32 and LDS at memory speed. Head h is live for
attention_decode_length(h, seq) keys, so the lengths are ragged. Its window is
`iters` (the capacity in units of 128 keys, 0: 8192), `bytes` (Q plus K plus
V, 0: 256 heads, 1 GiB of K and V) and `passes`; attention_decode_shape()
states the shape and the splits, attention_operands() the data (Q is its rows
0..15). It is verified, reports its clock and refuses the four options as the
attention kind does. SERVING_KINDS is every kind a child can be started as.

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
# The kind that is a whole GEMM, operands from memory through LDS to the
# matrix cores, and every kind including it.
GEMM_KINDS = ("gemm",)
EVERY_KIND = ALL_KINDS + GEMM_KINDS
# The pairs that say what a neighbour does to a tenant running a GEMM.
GEMM_PAIRS: Tuple[Tuple[str, str], ...] = (
    ("gemm", "gemm"), ("gemm", "stream"), ("stream", "gemm"), ("gemm", "fma"))
# The kinds that are a block-scaled GEMM, the form in the name; every kind
# there is; and the pairs that say what a neighbour does to such a tenant.
MXGEMM_KINDS = ("gemm-mxfp8", "gemm-mxfp4")
TENANT_KINDS = EVERY_KIND + MXGEMM_KINDS


def mxgemm_pairs(kind: str) -> Tuple[Tuple[str, str], ...]:
    """GEMM_PAIRS with `kind` (one of MXGEMM_KINDS) in place of "gemm"."""
    if kind not in MXGEMM_KINDS:
        raise ValueError(f"not a block-scaled gemm kind: {kind!r}")
    return tuple(tuple(kind if k == "gemm" else k for k in pair) for pair in GEMM_PAIRS)


# The kinds that are the decode shape of a block-scaled GEMM, the form in the
# name; and every kind a tenant can be.
DECODE_KINDS = ("decode-mxfp8", "decode-mxfp4")
CO_KINDS = TENANT_KINDS + DECODE_KINDS
DECODE_ROWS = 32  # rows of A


def decode_pairs(kind: str) -> Tuple[Tuple[str, str], ...]:
    """The pairs that say what a neighbour does to a decode tenant of `kind`
    (one of DECODE_KINDS) and what it does to them: another such tenant, the
    streamer both ways round, and the prefill bf16 GEMM both ways round."""
    if kind not in DECODE_KINDS:
        raise ValueError(f"not a decode kind: {kind!r}")
    return ((kind, kind), (kind, "stream"), ("stream", kind), (kind, "gemm"), ("gemm", kind))


# The kind that is a causal flash-attention forward pass, and every kind a
# child can be started as.
ATTENTION_KINDS = ("attention",)
WORKLOAD_KINDS = CO_KINDS + ATTENTION_KINDS
ATTENTION_HEAD_DIM = 128
# What |O - float64 reference| may be for an attention tenant's bf16 output:
# derived, not measured. With |v| <= 15/16 the rounding of P to bf16 moves an
# output by at most 2^-8 * 15/16 (truncation) or 2^-9 * 15/16 (nearest); the
# bf16 store of O adds at most another 2^-9 * 15/16; f32 accumulation over seq
# <= 32768 terms adds at most seq * 2^-24; and the exp2 argument carries at
# most 230 * 2^-23 of relative error into p. All of that is below 2^-7. A numpy
# emulation of the kernel's arithmetic (f32 exp2, P to bf16, f32 accumulate,
# bf16 store) at seq 128, 384 and 1024 stays within 0.0031 with truncation and
# 0.0024 with round-to-nearest, while dropping one K/V tile moves 99-100 % of
# the rows behind it beyond 2^-7 and a mask one key too wide 10-41 % of all
# rows. The decode shape keeps the derivation: its weights are normalised, |v|
# <= 15/16 holds, and the f32 merges of the waves and of the splits under their
# common maximum add nothing of size. The emulation was not re-run with the
# split merge; on the card the kernel's every-element tests at seq 128 .. 2176
# stayed within 0.0023.
ATTENTION_TOLERANCE = 2 ** -7


# The kind that is a decode step's attention (split-KV, K and V streamed once),
# and every kind a child can be started as.
ATTENTION_DECODE_KINDS = ("attention-decode",)
SERVING_KINDS = WORKLOAD_KINDS + ATTENTION_DECODE_KINDS
ATTENTION_DECODE_QUERIES = 16


def attention_decode_pairs() -> Tuple[Tuple[str, str], ...]:
    """The pairs that say what a neighbour does to an attention-decode tenant
    and what it does to them: another such tenant, the streamer, the prefill
    attention and the decode-mxfp4 GEMM, both ways round each."""
    kind, others = ATTENTION_DECODE_KINDS[0], ("stream", "attention", "decode-mxfp4")
    return ((kind, kind),) + tuple(
        pair for other in others for pair in ((kind, other), (other, kind)))


def attention_decode_shape(bytes: int = 0, iters: int = 0) -> Tuple[int, int, int, int]:
    """(heads, seq, 128, splits) of the step an attention-decode tenant runs
    for the window keys `bytes` and `iters`, the probe's rule stated on its
    own: seq = 128 * iters (0: 64; clamped to 1 .. 256), heads = bytes // (512 *
    seq + 4096), a key's row of K and of V being 512 bytes and a head's 16 rows
    of Q 4096 (0: 256 heads), clamped to 1 .. 1024, and splits = 2048 // heads
    clamped to 1 .. ceil(iters / 8); a split is ceil(iters / splits) units of
    128 keys."""
    units = min(int(iters), 256) if int(iters) > 0 else 64
    seq = 128 * units
    heads = int(bytes) // (512 * seq + 4096) if int(bytes) else 256
    heads = min(max(heads, 1), 1024)
    return heads, seq, ATTENTION_HEAD_DIM, min(max(2048 // heads, 1), -(-units // 8))


def attention_decode_length(head: int, seq: int) -> int:
    """The live keys of `head` of an attention-decode tenant: keys 0 .. this -
    1 count, the rest of the `seq` are in memory and must not."""
    return int(seq) - (37 * int(head)) % 128


def attention_pairs() -> Tuple[Tuple[str, str], ...]:
    """The pairs that say what a neighbour does to an attention tenant and
    what it does to them: another such tenant, the streamer, the prefill bf16
    GEMM and the decode-mxfp4 tenant (the prefill/decode mix of a serving
    node), both ways round each."""
    others = ("stream", "gemm", "decode-mxfp4")
    return (("attention", "attention"),) + tuple(
        pair for kind in others for pair in (("attention", kind), (kind, "attention")))


def attention_shape(bytes: int = 0, iters: int = 0) -> Tuple[int, int, int]:
    """(heads, seq, 128) of the forward pass an attention tenant runs for the
    window keys `bytes` and `iters`, the probe's rule stated on its own: seq =
    128 * iters (0: 64, seq 8192; clamped to 1 .. 256), and heads = bytes //
    (768 * seq), a row of Q, K and V being 768 bytes of bf16 (0: 64 heads),
    clamped to 1 .. 1024."""
    seq = 128 * (min(int(iters), 256) if int(iters) > 0 else 64)
    heads = int(bytes) // (768 * seq) if int(bytes) else 64
    return min(max(heads, 1), 1024), seq, ATTENTION_HEAD_DIM


def attention_operands(seed: int, head: int, seq: int
                       ) -> Tuple[List[List[float]], List[List[float]], List[List[float]]]:
    """Q, K and V ([seq][128] each) of `head` of an attention tenant, the
    probe's data rule stated on its own: key = mix32(mix32(seed32 ^ 0x4154544E)
    ^ which * 0x9E3779B1 ^ head) with which = 0, 1, 2, and the element at
    [row][d] is (mix32(key ^ (row << 7 | d)) % 31 - 15) / 8, / 4 or / 16, all
    exact in bf16."""
    base = _mix32((int(seed) & _M32) ^ 0x4154544E)
    out = []
    for which, scale in enumerate((8.0, 4.0, 16.0)):
        key = _mix32(base ^ (which * 0x9E3779B1 & _M32) ^ int(head))
        out.append([[(_mix32(key ^ (row << 7 | d)) % 31 - 15) / scale
                     for d in range(ATTENTION_HEAD_DIM)] for row in range(int(seq))])
    return out[0], out[1], out[2]


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


# How a gemm tenant's slabs reach LDS: through registers, or straight from
# memory with the LDS-DMA load.
GEMM_LOADS = ("registers", "direct")
# How a decode tenant's weights lie in memory: row-major, or shuffled once
# into the order its waves consume them.
DECODE_WEIGHTS = ("rows", "tiled")
# What an mfma, a gemm or a decode tenant may be told beyond its window, in
# the order its child is told, each with the values it may take and the kinds
# it is for.
_MFMA_OPTIONS = {"form": MFMA_FORMS, "operands": MFMA_OPERANDS, "loads": GEMM_LOADS,
                 "weights": DECODE_WEIGHTS}
_OPTION_KINDS = {"form": MATRIX_KINDS, "operands": MATRIX_KINDS, "loads": GEMM_KINDS,
                 "weights": DECODE_KINDS}


def _checked(key: str, value: Optional[str]) -> str:
    if value not in _MFMA_OPTIONS[key]:
        whose = _OPTION_KINDS[key][0].split("-")[0]  # mfma, gemm or decode
        raise ValueError(f"unknown {whose} {key} {value!r}: one of "
                         + ", ".join(_MFMA_OPTIONS[key]))
    return value


def _mfma_option(key: str, tenant: Mapping[str, Any], kind: str,
                 wide: Optional[str]) -> Optional[str]:
    """The option `key` that `tenant`, run as `kind`, is started with: its
    own, else the call-wide `wide`; None when neither names one."""
    own = tenant.get(key)
    if kind not in _OPTION_KINDS[key]:
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


# --- the gemm tenant's oracle -------------------------------------------------

GEMM_TILE = 128          # rows of A and of B per workgroup
GEMM_STEP = 64           # k per step: K = 64 * iters
GEMM_ROW_PERIOD = 192    # A[m][k] and B[n][k] repeat in m and n ...
GEMM_K_PERIOD = 96       # ... and in k
# Per form of a GEMM tenant ("bf16": the gemm kind; the others: "gemm-" + the
# form), as in csrc/gpuprobe/cotenant.hip: the k of one step, a slab row of
# 128 bytes in every form, the most steps whose sums stay exact in f32, and
# the bytes of a row's scales per step (one E8M0 byte per block of 32 k).
GEMM_FORM_TABLE: Dict[str, Dict[str, int]] = {
    "bf16": {"step": 64, "max_iters": 512, "scale_bytes": 0},
    "mxfp8": {"step": 128, "max_iters": 256, "scale_bytes": 4},
    "mxfp4": {"step": 256, "max_iters": 64, "scale_bytes": 8},
}


def _gemm_form(form: str) -> Dict[str, int]:
    if form not in GEMM_FORM_TABLE:
        raise ValueError(f"unknown gemm form {form!r}: one of " + ", ".join(GEMM_FORM_TABLE))
    return GEMM_FORM_TABLE[form]


def gemm_shape(bytes: int = 0, iters: int = 0, form: str = "bf16") -> Tuple[int, int, int]:
    """(m, n, k) of the GEMM a gemm tenant runs for the window keys `bytes`
    and `iters`, the probe's rule stated on its own: k = 64 * iters (0: 64
    steps; clamped to 1 .. 512), and m = n = bytes // (4 k), A plus B being
    4 m k bytes of bf16 (0: 128 MiB), rounded down to a multiple of 128 and
    clamped to 128 .. 32768.

    `form` "mxfp8" or "mxfp4" is the rule of the gemm-mxfp8 and gemm-mxfp4
    kinds: a step is 128 or 256 k (0: K = 4096; clamped to 1 .. 256 or 1 ..
    64 steps), and A plus B, the elements alone, are 2 m k or m k bytes, in
    every form 256 bytes per row and step (0: m = 8192)."""
    rule = _gemm_form(form)
    steps = min(int(iters), rule["max_iters"]) if int(iters) > 0 else 4096 // rule["step"]
    unset = 128 << 20 if form == "bf16" else 8192 * 256 * steps
    side = (int(bytes) or unset) // (256 * steps) // GEMM_TILE * GEMM_TILE
    side = min(max(side, GEMM_TILE), 32768)
    return side, side, rule["step"] * steps


def decode_shape(bytes: int = 0, iters: int = 0, form: str = "mxfp4") -> Tuple[int, int, int]:
    """(32, n, k) of the GEMM a decode-mxfp8 or decode-mxfp4 tenant (`form`
    "mxfp8" or "mxfp4") runs for the window keys `bytes` and `iters`, the
    probe's rule stated on its own: k = 128 or 256 * iters (0: K = 8192;
    clamped to 1 .. 256 or 1 .. 64 steps), and n = bytes // (128 * iters), W's
    elements being 128 bytes per row and step in either form (0: 1 GiB),
    rounded down to a multiple of 128 and clamped to 128 .. 2^20."""
    rule = _gemm_form(form)
    if not rule["scale_bytes"]:
        raise ValueError(f"a decode tenant is block-scaled: {form!r}")
    steps = min(int(iters), rule["max_iters"]) if int(iters) > 0 else 8192 // rule["step"]
    n = (int(bytes) or 1 << 30) // (128 * steps) // GEMM_TILE * GEMM_TILE
    return DECODE_ROWS, min(max(n, GEMM_TILE), 1 << 20), rule["step"] * steps


def gemm_checksum(m: int, n: int, k: int, passes: int, seed: int,
                  form: str = "bf16") -> int:
    """What a gemm tenant's checksum must be, in integers and closed form. C
    = A . B^T with A[i][kk] = a(i % 192, kk % 96) and B[j][kk] = b(kk % 96, j
    % 192), the bf16 hashes of the mfma oracle under key = mix32(seed32 ^
    0x47454D4D), all in -15 .. 15. Every entry C[i][j] is weighed by (1 + i)
    (1 + j), and pass p = 0 .. passes - 1 of the launch, each the same
    product, by 1 + p. With U(r) the sum of 1 + i over the i < m that are r
    modulo 192, V likewise over n, and cnt(kk) = k // 96 + (kk < k % 96) the
    k that are kk modulo 96, one GEMM folds to

        G = sum over kk < 96 of cnt(kk) * (sum_r U(r) a(r, kk))
                                        * (sum_r V(r) b(kk, r)),

    and the checksum is G * passes * (passes + 1) / 2 modulo 2^64: O(m + n +
    192 * 96) whatever the size.

    `form` "mxfp8" or "mxfp4" takes a and b from the hashes of that form,
    each element under the scale of its own block of 32 k, block (kk % 96)
    // 32 of the three in a k period: the effective integers of the mfma
    oracle, |a| <= 14 and |b| <= 14, or |a| <= 24 and |b| <= 12. G is the
    same expression."""
    _gemm_form(form)
    fid = MFMA_FORMS.index(form)
    key = _mix32((int(seed) & _M32) ^ 0x47454D4D)

    def weights(size: int) -> List[int]:
        out = [0] * GEMM_ROW_PERIOD
        for i in range(int(size)):
            out[i % GEMM_ROW_PERIOD] += 1 + i
        return out

    u, v = weights(m), weights(n)
    total = 0
    for kk in range(GEMM_K_PERIOD):
        cnt = int(k) // GEMM_K_PERIOD + (kk < int(k) % GEMM_K_PERIOD)
        total += (cnt * sum(u[r] * _mfma_a(key, r, kk, fid) for r in range(GEMM_ROW_PERIOD))
                  * sum(v[r] * _mfma_b(key, kk, r, fid) for r in range(GEMM_ROW_PERIOD)))
    return total * (int(passes) * (int(passes) + 1) // 2) % (1 << 64)


# --- child ------------------------------------------------------------------

def _child_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="cotenancy", description=__doc__)
    p.add_argument("--child", action="store_true", required=True)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--kind", choices=SERVING_KINDS, default="fma")
    p.add_argument("--launches", type=int, default=8)
    p.add_argument("--iters", type=int, default=0)
    p.add_argument("--bytes", type=int, default=0)
    p.add_argument("--passes", type=int, default=0)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--form", choices=MFMA_FORMS, default="bf16")
    p.add_argument("--operands", choices=MFMA_OPERANDS, default=None)
    p.add_argument("--loads", choices=GEMM_LOADS, default=None)
    p.add_argument("--weights", choices=DECODE_WEIGHTS, default=None)
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
    # And the gemm kind's loads: the probe refuses "direct" beside another kind.
    if args.loads is not None:
        window["loads"] = args.loads
    # And the decode kinds' weights: the probe refuses "tiled" beside another kind.
    if args.weights is not None:
        window["weights"] = args.weights
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
             operands: Optional[str] = None,
             loads: Optional[str] = None,
             weights: Optional[str] = None) -> Dict[str, Any]:
    """Run up to two tenants at once on `card`, each a fresh child process
    under ROC_GLOBAL_CU_MASK = its mask. A tenant is {"mask": int, "kind":
    "fma" | "stream" | "cache" | "chase" | "mfma" | "gemm" | "gemm-mxfp8" |
    "gemm-mxfp4" | "decode-mxfp8" | "decode-mxfp4" | "attention" |
    "attention-decode"} and may
    carry its own "launches", "iters",
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
    for it. A gemm, gemm-mxfp8, gemm-mxfp4 or decode tenant is of another
    kind in this sense: it takes neither.

    `loads` (one of GEMM_LOADS) says how every gemm tenant of the call gets
    its slabs into LDS, by the same rules again: a gemm tenant may carry its
    own "loads" instead, an unknown value or "loads" on a tenant of any
    other kind (gemm-mxfp8, gemm-mxfp4 and the decode kinds included)
    raises ValueError before
    anything is started, the call-wide value leaves the other kinds as they
    are, and a child is given --loads, after --operands, only when one was
    named for it.

    `weights` (one of DECODE_WEIGHTS) says how every decode tenant of the
    call finds its weight matrix in memory, by the same rules once more: a
    decode tenant may carry its own "weights" instead, an unknown value or
    "weights" on a tenant of any other kind raises ValueError before
    anything is started, the call-wide value leaves the other kinds as they
    are, and a child is given --weights, after --loads, only when one was
    named for it. An attention or attention-decode tenant takes none of the
    four: its child is started with its window alone.

    Each child has `timeout` seconds from its start. The first child that
    times out, exits non-zero or prints no TENANT line ends the run: the
    others are killed and {"ok": False, "reason": "child-failed", "detail"}
    is returned. Nothing is retried."""
    if not 1 <= len(tenants) <= 2:
        raise ValueError("run_pair takes one or two tenants")
    if kinds is not None and len(kinds) != len(tenants):
        raise ValueError("one kind per tenant")
    call = {"form": form, "operands": operands, "loads": loads, "weights": weights}
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
            if kind not in SERVING_KINDS:
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
_SOLO_KEYS = {"chase": ("ns_per_hop",), "mfma": ("clock_ghz",), "gemm": ("clock_ghz",),
              **{kind: ("clock_ghz",) for kind in MXGEMM_KINDS + DECODE_KINDS},
              "attention": ("clock_ghz",), "attention-decode": ("clock_ghz",)}


def _expected(result: Mapping[str, Any], seed: int, pattern, form=None,
              operands=None, loads=None, weights=None) -> Optional[int]:
    """The checksum a child's result must carry by the oracle of its kind
    (`pattern` is the reading kinds'); None for a kind that has none. A gemm
    tenant's `loads` and a decode tenant's `weights` do not enter it: the
    product is the same."""
    kind = result["kind"]
    if kind in READING_KINDS:
        return pattern(seed, int(result["bytes"]))
    if kind == "chase":
        return chase_checksum(result["bytes"], result["workgroups"], result["iters"], seed)
    if kind in MATRIX_KINDS:
        return mfma_checksum(result["workgroups"], result["iters"], seed,
                             form or MFMA_FORMS[0], operands or MFMA_OPERANDS[0])
    if kind in GEMM_KINDS:
        return gemm_checksum(result["m"], result["n"], result["k"], result["passes"], seed)
    if kind in MXGEMM_KINDS:
        return gemm_checksum(result["m"], result["n"], result["k"], result["passes"], seed,
                             form=kind[len("gemm-"):])
    if kind in DECODE_KINDS:
        return gemm_checksum(result["m"], result["n"], result["k"], result["passes"], seed,
                             form=kind[len("decode-"):])
    return None


def isolation_report(card: int, tenants: Sequence[Mapping[str, Any]], *,
                     pairs: Sequence[Tuple[str, str]] = ALL_PAIRS,
                     launches: int = 8, iters: int = 0, bytes: int = 0,
                     passes: int = 0, seed: int = 1, timeout: float = 120.0,
                     spawn: Optional[Callable[..., Any]] = None,
                     expected_checksum: Optional[Callable[[int, int], int]] = None,
                     windows: Optional[Mapping[str, Mapping[str, int]]] = None,
                     form: Optional[str] = None,
                     operands: Optional[str] = None,
                     loads: Optional[str] = None,
                     weights: Optional[str] = None) -> Dict[str, Any]:
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

    A gemm tenant (pairs=GEMM_PAIRS) takes `bytes` (A plus B), `iters`
    (steps of 64 k) and `passes` (whole GEMMs per launch), see gemm_shape();
    its rates are GFLOP/s and its checksum is held against gemm_checksum().
    Its entries carry the clock and its split exactly as an mfma tenant's
    do: beside a streamer clock_ratio is what the chip-wide clock took and
    cycle_ratio what the shared memory path took. It takes neither `form`
    nor `operands`; one on a gemm tenant raises ValueError.

    A gemm-mxfp8 or gemm-mxfp4 tenant (pairs=mxgemm_pairs(kind)) is the
    same with block-scaled operands: `iters` are steps of 128 or 256 k,
    `bytes` the elements of A plus B, see gemm_shape(form=); its checksum is
    held against gemm_checksum(form=), and its entries carry the clock and
    its split as a gemm tenant's do. It too takes neither `form` nor
    `operands`.

    A decode-mxfp8 or decode-mxfp4 tenant (pairs=decode_pairs(kind)) is the
    decode shape of that GEMM, 32 rows of A against a weight matrix W that
    is streamed from memory once per pass: `bytes` are W's elements, `iters`
    steps of 128 or 256 k, `passes` re-reads of W, see decode_shape(). Its
    rates are GFLOP/s, 64 (mxfp8) or 128 (mxfp4) flop per byte of W, so rate
    / 64 or / 128 is the GB/s of weights it streams; its checksum is held
    against gemm_checksum(32, n, k, ..., form=), and its
    entries carry the clock and its split as a gemm tenant's do: beside a
    streamer or a prefill GEMM, clock_ratio is what the chip-wide clock took
    and cycle_ratio what the shared memory path took. It takes neither
    `form` nor `operands` nor `loads`.

    An attention tenant (pairs=attention_pairs()) is a causal
    flash-attention forward pass in bf16: `iters` is the sequence length in
    units of 128 rows, `bytes` Q plus K plus V, `passes` whole forward passes
    per launch, see attention_shape(). Its rates are GFLOP/s over the
    unmasked half of Q K^T and P V. It has no checksum; its result carries
    max_error, the largest difference between its output and the probe's
    fp64 reference over 256 sampled rows, and a max_error above
    ATTENTION_TOLERANCE makes the report not ok with reason "bad-output",
    the figures kept as for "bad-checksum". Its entries carry the clock and
    its split as a gemm tenant's do. It takes none of `form`, `operands`,
    `loads` and `weights`.

    An attention-decode tenant (pairs=attention_decode_pairs()) is a decode
    step's attention, 16 query rows against K and V streamed once per pass:
    `iters` is the capacity in units of 128 keys, `bytes` Q plus K plus V,
    `passes` whole steps per launch, see attention_decode_shape(). Its rates
    are GFLOP/s, 4 x 128 x 16 flop per live key, that is 16 flop per byte of K
    and V, so rate / 16 is the GB/s it streams. Verified, split into clock and
    cycles and refused the four options as an attention tenant is.

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

    `loads` (one of GEMM_LOADS, anything else raises ValueError) says how
    the gemm tenants get their slabs into LDS, alone and in every pair:
    "registers", or "direct" for tenants that load them straight from
    memory into a ring of LDS buffers; a tenant ({"mask": int, "loads":
    str}) may name its own instead. The other kinds are not touched by it.
    The checksum stays gemm_checksum()'s, and the gemm entries, solo and in
    a pair, add "loads". With none named anywhere the children are started
    as before and no entry has "loads".

    `weights` (one of DECODE_WEIGHTS, anything else raises ValueError) says
    how the decode tenants' weight matrix lies in memory, alone and in every
    pair: "rows", row-major, or "tiled", shuffled once into the order the
    waves consume it, as production decode GEMMs keep their weights, so that
    every load instruction reads whole lines; a tenant ({"mask": int,
    "weights": str}) may name its own instead. The other kinds are not
    touched by it. The checksum stays gemm_checksum(32, n, k, ..., form=)'s,
    and the decode entries, solo and in a pair, add "weights". With none
    named anywhere the children are started as before and no entry has
    "weights".

    ok says that the measurement is valid (every child exited 0, every
    stream and cache checksum equals the pattern's, every chase, mfma and
    gemm checksum the closed form's, overlap was reached), not that the
    tenants are isolated: no interference threshold is built in, on ratio,
    clock_ratio or cycle_ratio. The first
    child that fails ends the report ("child-failed"): nothing further is
    started."""
    if len(tenants) != 2:
        raise ValueError("isolation_report takes two tenants")
    for pair in pairs:
        if len(pair) != 2 or any(k not in SERVING_KINDS for k in pair):
            raise ValueError(f"not a pair of tenant kinds: {pair!r}")
    windows = {kind: dict(w) for kind, w in (windows or {}).items()}
    for kind, w in windows.items():
        if kind not in SERVING_KINDS or any(k not in WINDOW_KEYS for k in w):
            raise ValueError(f"not a window of a tenant kind: {kind!r}: {w!r}")
    # Per option and tenant, what the tenant is started with as a tenant of
    # the option's kind.
    named = {key: [_mfma_option(key, t, _OPTION_KINDS[key][0], wide) for t in tenants]
             for key, wide in (("form", form), ("operands", operands), ("loads", loads),
                               ("weights", weights))}
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
        # An attention tenant has no checksum: the probe's own fp64 reference
        # says how far its output is off (a not-a-number is not within).
        if result["kind"] in ATTENTION_KINDS + ATTENTION_DECODE_KINDS and not (
                result["max_error"] <= ATTENTION_TOLERANCE):
            return "bad-output"
        return None

    for i, tenant in enumerate(tenants):
        for kind in SERVING_KINDS:
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
