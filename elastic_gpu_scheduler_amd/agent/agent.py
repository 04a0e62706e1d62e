"""MI355X node agent: publishes inventory + xGMI topology, verifies health
and placement.

The reference repo relies on a sibling project (elastic-gpu-agent, NVML +
nvidia-docker) for the node side; this module is the MI355X-native
equivalent's control logic:

  * publish() — writes the per-card inventory and the xGMI hop matrix onto
    the Node object as annotations (elasticgpu.io/gpu-inventory,
    elasticgpu.io/xgmi-topology); the scheduler's node cache consumes them
    (k8s.objects.node_devices / node_topology). The whole-card-count
    extended resource itself is advertised by the ROCm k8s device plugin
    (amd.com/gpu); gpu-core/gpu-memory allocatable are derived from the
    published inventory;
  * health_check() — runs the HIP HBM-bandwidth probe per card and flags
    cards below a threshold (a sick HBM stack or wrong partition mode);
  * self_test() — the deep, opt-in version: HBM pattern test, per-XCD read
    bandwidth and an MFMA check per card, judged by agent/health.py;
  * verify_placement() — stamps a pod-unique tag on the cards a bound pod
    was assigned, proving the scheduler/device-plugin contract held
    (BASELINE.json: "rocprof/amd-smi spot-check that containers land on the
    chosen card indices" — this is the programmatic version);
  * assign_masks() / sync_masks() / verify_masks() — gpu-core enforcement:
    each fractional container gets a CU mask sized to its share
    (agent/cumask.py), recorded on the pod as elasticgpu.io/cu-mask and
    turned into the container's environment by agent/wiring.py;
    verify_masks() proves on the card that the masks confine work to
    disjoint physical CUs;
  * verify_isolation() — a qualification run for an idle card: two tenants
    in separate processes under disjoint masks, each one's rate alone and
    next to the other (agent/cotenancy.py);
  * cache_profile() — likewise for an idle card: one tenant alone, its
    re-read rate by working-set size, which shows where the caches end;
  * chase_profile() — likewise: one tenant alone, its time per dependent
    load by working-set size, the latency of each level of the hierarchy.
"""
from __future__ import annotations

import json
import logging
import time
from typing import Any, Dict, List, Optional, Sequence

from elastic_gpu_scheduler_amd.agent import inventory as inv
from elastic_gpu_scheduler_amd.agent import topology as topo
from elastic_gpu_scheduler_amd.agent.cumask import (CardMaskPlan, MaskGrant,
                                                    mask_hex, parse_mask_hex)
from elastic_gpu_scheduler_amd.agent.health import HealthLimits, evaluate_card
from elastic_gpu_scheduler_amd.agent.wiring import fractional_core, pod_cu_masks
from elastic_gpu_scheduler_amd.k8s import objects as obj
from elastic_gpu_scheduler_amd.k8s.client import KubeClient
from elastic_gpu_scheduler_amd.utils import types as t

log = logging.getLogger("egs.agent")

# A healthy MI355X streams HBM3E far above 1 TB/s (measured ceiling ~6.3 TB/s
# for a float4 copy); anything below this is a sick card or a misconfigured
# partition and should not be scheduled onto.
HBM_HEALTH_THRESHOLD_GBPS = 1000.0

# Seed of the deep self-test's HBM pattern (any value serves; fixed so a
# reported word index and XOR can be reproduced).
SELF_TEST_PATTERN_SEED = 0x6A09E667F3BCC908

# Working sets of cache_profile(): below, around and above the aggregate L2
# (32 MiB) and the Infinity Cache (256 MiB).
CACHE_PROFILE_SIZES = tuple(m << 20 for m in (2, 8, 16, 24, 48, 128, 192, 512, 1024))

# Working sets of chase_profile(): every XCD walks the whole buffer, so the
# steps are at one XCD's L2 (4 MiB) and the Infinity Cache (256 MiB).
CHASE_PROFILE_SIZES = tuple(m << 20 for m in (1, 2, 4, 8, 32, 64, 128, 256, 512, 1024))


class NodeAgent:
    def __init__(self, node_name: str, client: Optional[KubeClient] = None,
                 prefer_source: str = "auto") -> None:
        self.node_name = node_name
        self.client = client
        self.prefer_source = prefer_source
        # cards the most recent deep self-test found unhealthy
        self._deep_sick: set = set()
        # CU-mask state: measured layouts, one plan per card, entries per pod
        self._mask_layouts: Optional[Dict[int, Dict[str, Any]]] = None
        self._mask_plans: Dict[int, CardMaskPlan] = {}
        self._pod_masks: Dict[str, Dict[str, Dict[str, Any]]] = {}

    # -- discovery --

    def snapshot(self) -> Dict[str, Any]:
        cards = inv.discover(self.prefer_source)
        hops = topo.discover(len(cards), self.prefer_source)
        return {"cards": cards, "topology": {"hops": hops}}

    def annotations(self) -> Dict[str, str]:
        snap = self.snapshot()
        return {
            t.ANNOTATION_NODE_INVENTORY: json.dumps({"cards": snap["cards"]}),
            t.ANNOTATION_NODE_TOPOLOGY: json.dumps(snap["topology"]),
        }

    def allocatable(self) -> Dict[str, str]:
        """The elasticgpu.io allocatable a device plugin would advertise for
        this node, derived from the live inventory."""
        snap = self.snapshot()
        cards = snap["cards"]
        total_core = sum(c.get("core", t.GPU_CORE_EACH_CARD) for c in cards)
        total_mem = sum(int(c.get("memory_bytes", 0)) for c in cards)
        return {
            t.RESOURCE_GPU_CORE: str(total_core),
            t.RESOURCE_GPU_MEMORY: str(total_mem),
            t.RESOURCE_AMD_GPU: str(len(cards)),
        }

    def publish(self) -> Dict[str, str]:
        """Publish inventory/topology annotations AND the elasticgpu.io
        allocatable quantities onto the Node (the role the reference
        delegates to its device plugin's node updates)."""
        if self.client is None:
            raise RuntimeError("NodeAgent.publish needs a KubeClient")
        ann = self.annotations()
        self.client.patch_node_annotations(self.node_name, ann)
        try:
            self.client.patch_node_allocatable(self.node_name,
                                               self.allocatable())
        except NotImplementedError:
            pass  # client without status-subresource support
        return ann

    def publish_with_health(self, mib: int = 256, iters: int = 5,
                            deep: bool = False) -> Dict[str, Any]:
        """Publish inventory with unhealthy cards EXCLUDED (HBM bandwidth
        below threshold): the scheduler stops placing onto sick cards at the
        next node-cache refresh. Returns {"published": ann, "sick": [...]}.

        deep=True gates on self_test() instead of the bandwidth probe alone
        and also publishes the per-card verdicts as the
        elasticgpu.io/gpu-health annotation. A card the last deep run found
        bad stays excluded through the plain cycles in between: a bandwidth
        probe cannot clear a data or matrix-core error.
        """
        if self.client is None:
            raise RuntimeError("publish_with_health needs a KubeClient")
        if deep:
            report = self.self_test()
            self._deep_sick = {r["index"] for r in report if not r["healthy"]}
        else:
            report = self.health_check(mib=mib, iters=iters)
        sick = [r["index"] for r in report if not r["healthy"]]
        if not deep and self._deep_sick:
            sick = sorted(set(sick) | self._deep_sick)
        ann = self.annotations()
        if deep:
            ann[t.ANNOTATION_NODE_HEALTH] = json.dumps(
                {"cards": [health_summary(r) for r in report]},
                separators=(",", ":"))
        inv = json.loads(ann[t.ANNOTATION_NODE_INVENTORY])
        # Sick cards stay in the list as zero-capacity placeholders so list
        # position keeps equalling the PHYSICAL card index — dropping an
        # entry would shift every later card's index and the scheduler's
        # annotations (consumed as physical indexes by the device plugin)
        # would map pods onto the wrong card, including the sick one.
        # Zero-capacity devices are never schedulable (csrc/core/types.h
        # Device::schedulable).
        inv["cards"] = [
            ({**c, "core": 0, "memory_bytes": 0, "sick": True}
             if c["index"] in sick else c)
            for c in inv["cards"]
        ]
        ann[t.ANNOTATION_NODE_INVENTORY] = json.dumps(inv)
        self.client.patch_node_annotations(self.node_name, ann)
        try:
            alloc = {
                t.RESOURCE_GPU_CORE: str(sum(c.get("core", 100)
                                             for c in inv["cards"])),
                t.RESOURCE_GPU_MEMORY: str(sum(int(c.get("memory_bytes", 0))
                                               for c in inv["cards"])),
                t.RESOURCE_AMD_GPU: str(sum(1 for c in inv["cards"]
                                            if not c.get("sick"))),
            }
            self.client.patch_node_allocatable(self.node_name, alloc)
        except NotImplementedError:
            pass
        return {"published": ann, "sick": sick}

    def node_object(self) -> Dict[str, Any]:
        """A complete Node object for offline/bench use (fake apiserver)."""
        return {
            "metadata": {"name": self.node_name, "annotations": self.annotations()},
            "status": {"allocatable": self.allocatable()},
        }

    # -- GPU-side verification (requires the HIP probe + a visible GPU) --

    def health_check(self, mib: int = 256, iters: int = 5) -> List[Dict[str, Any]]:
        from elastic_gpu_scheduler_amd._native import gpuprobe

        probe = gpuprobe()
        out = []
        for i in range(probe.device_count()):
            bw = probe.hbm_bandwidth(i, mib, iters)
            out.append({"index": i, "hbm_gbps": bw,
                        "healthy": bw >= HBM_HEALTH_THRESHOLD_GBPS})
        return out

    def self_test(self, pattern_mib: int = 1024, slice_mib: int = 128,
                  mfma_iters: int = 256) -> List[Dict[str, Any]]:
        """Deep per-card self-test: the bandwidth probe plus the HBM pattern
        test, per-XCD read bandwidth and the MFMA check. One report per card:
        {index, hbm_gbps, pattern, xcd, mfma, healthy, reasons}.

        The defaults are the health settings: a pattern buffer must be well
        above the 256 MiB Infinity Cache for its verify pass to read HBM
        cells (smaller sizes only test the kernels and the caches), and
        8 x 128 MiB of XCD slices stream from HBM for the same reason. A run
        allocates about 1 GiB at a time on the card and saturates it for a
        moment, so it is not something to run every cycle next to tenants.
        """
        from elastic_gpu_scheduler_amd._native import gpuprobe

        probe = gpuprobe()
        slice_mib = slice_mib if 0 < slice_mib <= 512 else 128
        slice_words = slice_mib * 1024 * 1024 // 8
        chunk_kib = 256
        limits = HealthLimits(hbm_gbps=HBM_HEALTH_THRESHOLD_GBPS)
        out = []
        for i in range(probe.device_count()):
            report: Dict[str, Any] = {
                "index": i,
                "hbm_gbps": probe.hbm_bandwidth(i, 256, 5),
                "pattern": probe.hbm_pattern_test(
                    i, pattern_mib * 1024 * 1024, SELF_TEST_PATTERN_SEED),
                "xcd": _xcd_or_skipped(probe, i, slice_mib, chunk_kib),
                "mfma": probe.mfma_selftest(i, mfma_iters),
            }
            for e in ([] if "skipped" in report["xcd"] else report["xcd"]):
                e["expected_chunks"] = slice_mib * 1024 // chunk_kib
                e["expected_checksum"] = probe.pattern_xor(
                    probe.XCD_PATTERN_SEED, e["xcc"] * slice_words, slice_words)
            report.update(evaluate_card(report, limits))
            out.append(report)
        return out

    def verify_placement(self, pod_uid: str, device_indexes: List[int],
                         mib: int = 16) -> bool:
        """Stamp+verify a pod-unique pattern on each assigned card."""
        from elastic_gpu_scheduler_amd._native import gpuprobe

        probe = gpuprobe()
        tag = _uid_tag(pod_uid)
        return all(probe.stamp(idx, tag, mib) for idx in device_indexes)

    def measured_topology(self, mib: int = 64, iters: int = 5) -> Dict[str, Any]:
        """Measured xGMI bandwidth matrix (GB/s) alongside the hop matrix.
        On a healthy single-hive OAM board every off-diagonal pair should
        sustain a similar per-link bandwidth (~150 GB/s class per link)."""
        from elastic_gpu_scheduler_amd._native import gpuprobe

        probe = gpuprobe()
        n = probe.device_count()
        bw = [[0.0] * n for _ in range(n)]
        for i in range(n):
            for j in range(n):
                if i != j:
                    bw[i][j] = probe.p2p_bandwidth(i, j, mib, iters)
        return {"hops": probe.xgmi_hop_matrix(), "bandwidth_gbps": bw}

    # -- gpu-core enforcement: per-container CU masks --

    def mask_layouts(self) -> Dict[int, Dict[str, Any]]:
        """How CU-mask bits map to XCDs on each card (the probe's
        cu_mask_layout), measured once and cached."""
        if self._mask_layouts is None:
            from elastic_gpu_scheduler_amd._native import gpuprobe

            probe = gpuprobe()
            self._mask_layouts = {i: probe.cu_mask_layout(i)
                                  for i in range(probe.device_count())}
        return self._mask_layouts

    def mask_plan(self, card: int) -> Optional[CardMaskPlan]:
        """The card's mask plan; None when its layout is unknown or not
        interleaved: no masks are planned for such a card."""
        plan = self._mask_plans.get(card)
        if plan is None:
            layout = self.mask_layouts().get(card)
            if not layout or not layout.get("interleaved"):
                return None
            plan = CardMaskPlan(int(layout["cus"]), int(layout["granule"]))
            self._mask_plans[card] = plan
        return plan

    def assign_masks(self, pod: Dict[str, Any]) -> Dict[str, Dict[str, Any]]:
        """Grant a CU mask to each fractional container of a placed pod:
        {container: {card, mask, cus, shared}}. Idempotent per pod uid. Masks
        the pod's annotation already records are adopted as they are (its
        containers may be running under them); otherwise new ones are
        granted and, with a client, written to the pod as the
        elasticgpu.io/cu-mask annotation."""
        uid = obj.pod_uid(pod)
        if uid in self._pod_masks:
            return self._pod_masks[uid]
        allocation = obj.parse_allocation(pod)
        if allocation is None:
            return {}
        recorded = pod_cu_masks(pod)
        entries: Dict[str, Dict[str, Any]] = {}
        containers = pod.get("spec", {}).get("containers", []) or []
        for i, c in enumerate(containers):
            name = c.get("name", str(i))
            share = fractional_core(c)
            if not share or len(allocation[i]) != 1:
                continue
            plan = self.mask_plan(allocation[i][0])
            if plan is None:
                continue
            key = f"{uid}/{name}"
            old = recorded.get(name)
            if old is not None and old["card"] == allocation[i][0]:
                try:
                    plan.restore({key: MaskGrant(parse_mask_hex(old["mask"]),
                                                 old["cus"], old["shared"])})
                except ValueError:
                    log.warning("pod %s: unusable recorded cu-mask %r",
                                obj.pod_key(pod), old["mask"])
                    continue
                grant = plan.grants()[key]
            else:
                grant = plan.allocate(key, share)
            entries[name] = {"card": allocation[i][0],
                             "mask": mask_hex(grant.mask),
                             "cus": grant.cus, "shared": grant.shared}
        if not entries:
            return {}
        self._pod_masks[uid] = entries
        if self.client is not None and entries != recorded:
            try:
                self._write_mask_annotation(pod, entries)
            except Exception:
                self.release_masks(uid)  # nothing was promised to anyone yet
                raise
        return entries

    def _write_mask_annotation(self, pod: Dict[str, Any],
                               entries: Dict[str, Dict[str, Any]]) -> None:
        from elastic_gpu_scheduler_amd.k8s.client import ConflictError

        raw = json.dumps(entries, separators=(",", ":"), sort_keys=True)
        for attempt in range(3):
            fresh = self.client.get_pod(obj.pod_namespace(pod), obj.pod_name(pod))
            fresh.setdefault("metadata", {}).setdefault(
                "annotations", {})[t.ANNOTATION_POD_CU_MASK] = raw
            try:
                self.client.update_pod(fresh)
                return
            except ConflictError:
                if attempt == 2:
                    raise

    def release_masks(self, pod_uid: str) -> None:
        for name, e in self._pod_masks.pop(pod_uid, {}).items():
            plan = self._mask_plans.get(e["card"])
            if plan is not None:
                plan.release(f"{pod_uid}/{name}")

    def sync_masks(self) -> Dict[str, Dict[str, Dict[str, Any]]]:
        """Bring the plans in line with the pods placed on this node: adopt
        the masks existing annotations record first, then grant masks to the
        pods that have none, then free those of pods that are gone or
        completed. Returns {pod uid: mask entries}."""
        if self.client is None:
            raise RuntimeError("NodeAgent.sync_masks needs a KubeClient")
        live = []
        for pod in self.client.list_pods():
            ann = pod.get("metadata", {}).get("annotations", {}) or {}
            if (ann.get(t.ANNOTATION_EGPU_NODE) == self.node_name
                    and not obj.is_completed_pod(pod)):
                live.append(pod)
        live.sort(key=lambda p: (obj.pod_key(p), obj.pod_uid(p)))
        for recorded_first in (True, False):
            for pod in live:
                if bool(pod_cu_masks(pod)) == recorded_first:
                    self.assign_masks(pod)
        uids = {obj.pod_uid(p) for p in live}
        for uid in [u for u in self._pod_masks if u not in uids]:
            self.release_masks(uid)
        return dict(self._pod_masks)

    def verify_masks(self, card: int) -> Dict[str, Any]:
        """Run the occupancy probe under every grant on `card`. Each grant
        must show as many physical CUs as its mask has bits, equally many on
        every XCD, and grants not marked shared must be pairwise disjoint in
        physical CUs. Returns {"ok", "overlaps", "per_grant"}. Nothing is
        launched under a mask on a card whose layout is not interleaved, or
        under a mask that is not whole granules."""
        from elastic_gpu_scheduler_amd._native import gpuprobe

        layout = self.mask_layouts().get(card)
        plan = self.mask_plan(card)
        if not layout or plan is None:
            return {"ok": False, "reason": "unsupported-layout"}
        probe = gpuprobe()
        xccs = int(layout["xccs"])
        seen: Dict[Any, set] = {}
        per_grant: Dict[Any, Dict[str, Any]] = {}
        grants = plan.grants()
        for key, grant in grants.items():
            if not plan.whole_granules(grant.mask):
                per_grant[key] = {"ok": False, "reason": "not-whole-granules"}
                continue
            occ = probe.cu_occupancy(card, mask=grant.mask)
            cus = {(e["xcc"], e["se"], e["sh"], e["cu"]) for e in occ["cus"]}
            per_xcc: Dict[int, int] = {}
            for k in cus:
                per_xcc[k[0]] = per_xcc.get(k[0], 0) + 1
            seen[key] = cus
            per_grant[key] = {
                "ok": (occ["applied_mask"] == grant.mask
                       and len(cus) == grant.cus and len(per_xcc) == xccs
                       and set(per_xcc.values()) == {grant.cus // xccs}),
                "mask": mask_hex(grant.mask), "cus": len(cus),
                "per_xcc": dict(sorted(per_xcc.items())),
                "shared": grant.shared,
            }
        overlaps = []
        keys = [k for k in seen if not grants[k].shared]
        for i, a in enumerate(keys):
            for b in keys[i + 1:]:
                both = seen[a] & seen[b]
                if both:
                    overlaps.append({"a": a, "b": b, "cus": sorted(both)})
        return {"ok": not overlaps and all(g["ok"] for g in per_grant.values()),
                "overlaps": overlaps, "per_grant": per_grant}

    def verify_isolation(self, card: int, shares=(50, 50),
                         **window: Any) -> Dict[str, Any]:
        """Two tenants holding `shares` percent of `card`, run as separate
        processes under the masks the planner would grant them, exactly as
        containers are wired: each tenant's FMA and HBM-stream rate alone and
        while the other runs (cotenancy.isolation_report, to which `window`
        is passed: pairs, launches, iters, bytes, passes, timeout, windows,
        form, operands).
        Returns that report plus "tenants": [{core, mask, cus}].

        pairs=cotenancy.CACHE_PAIRS brings in the third kind, a tenant that
        re-reads a working set small enough for a cache; `windows` gives a
        kind its own iters / bytes / passes, e.g. {"cache": {"bytes": 12 <<
        20, "passes": cotenancy.cache_passes(12 << 20)}} next to the default
        1 GiB streamer. pairs=cotenancy.CHASE_PAIRS brings in the fourth, a
        tenant bound by the latency of dependent loads, e.g. with windows=
        {"chase": {"bytes": 64 << 20}}; its rates are Ghop/s and its solo
        entry adds ns_per_hop. pairs=cotenancy.MFMA_PAIRS brings in the
        fifth, a tenant issuing bf16 MFMAs back to back from registers: the
        one load under which the chip lowers its clock for every tenant,
        whatever the masks. Its rates are GFLOP/s, its solo entry adds
        clock_ghz, and its entry in a pair splits ratio into clock_ratio
        (what the shader clock explains) and cycle_ratio (what it does not).
        form= (one of cotenancy.MFMA_FORMS: "bf16", "fp8", "mxfp8", "mxfp4")
        names the instruction the mfma tenants issue in place of the bf16
        one; their entries then add "form". For two tenants of different
        forms, such as bf16 beside mxfp4, call cotenancy.isolation_report
        with a "form" in each tenant. operands= (one of
        cotenancy.MFMA_OPERANDS: "registers", "lds") says where the mfma
        tenants take their operands from: "lds" makes them re-read every
        step's operands from LDS, as a GEMM does, in place of keeping them
        in registers; their entries then add "operands".

        The masks come from a scratch plan over the measured layout; the
        live plan is not touched. As in verify_masks, nothing is launched
        when the layout is unknown or not interleaved, or under a mask that
        is not whole granules ("unsupported-layout"); shares that cannot
        both be met from free granules are refused ("shares-overlap").

        This is a qualification run for an idle card: it saturates the card
        for about a second per pair and would itself be the noisy neighbour
        of any tenant running there. "ok" says the measurement is valid, not
        that the tenants are isolated."""
        from elastic_gpu_scheduler_amd.agent import cotenancy

        if len(shares) != 2:
            raise ValueError("verify_isolation takes two shares")
        layout = self.mask_layouts().get(card)
        if not layout or not layout.get("interleaved"):
            return {"ok": False, "reason": "unsupported-layout"}
        try:
            plan = CardMaskPlan(int(layout["cus"]), int(layout["granule"]))
        except ValueError:
            return {"ok": False, "reason": "unsupported-layout"}
        grants = [plan.allocate(i, int(core)) for i, core in enumerate(shares)]
        if not all(plan.whole_granules(g.mask) for g in grants):
            return {"ok": False, "reason": "unsupported-layout"}
        tenants = [{"core": int(core), "mask": mask_hex(g.mask), "cus": g.cus}
                   for core, g in zip(shares, grants)]
        if any(g.shared for g in grants) or grants[0].mask & grants[1].mask:
            return {"ok": False, "reason": "shares-overlap", "tenants": tenants}
        report = cotenancy.isolation_report(
            card, [{"mask": g.mask} for g in grants], **window)
        report["tenants"] = tenants
        return report

    def cache_profile(self, card: int, share: int = 50,
                      sizes: Sequence[int] = CACHE_PROFILE_SIZES,
                      **window: Any) -> Dict[str, Any]:
        """One tenant holding `share` percent of `card`, alone, re-reading
        working sets of `sizes` bytes (default 2 MiB .. 1 GiB), one process
        per size under the mask the planner would grant it: where the rate
        steps down, the working set has left a cache (cotenancy.
        cache_profile, to which `window` is passed: launches, passes,
        timeout). Returns that report plus "tenant": {core, mask, cus}.

        Gated as verify_isolation is: a scratch plan over the measured
        layout, and nothing is launched when the layout is unknown or not
        interleaved or the mask is not whole granules
        ("unsupported-layout"). For an idle card."""
        from elastic_gpu_scheduler_amd.agent import cotenancy

        return self._solo_profile(cotenancy.cache_profile, card, share, sizes, window)

    def chase_profile(self, card: int, share: int = 50,
                      sizes: Sequence[int] = CHASE_PROFILE_SIZES,
                      **window: Any) -> Dict[str, Any]:
        """One tenant holding `share` percent of `card`, alone, following a
        chain of dependent loads through working sets of `sizes` bytes
        (default 1 MiB .. 1 GiB), one process per size under the mask the
        planner would grant it: where the time per hop steps up, the working
        set has left a cache (cotenancy.chase_profile, to which `window` is
        passed: launches, iters, timeout). Returns that report plus
        "tenant": {core, mask, cus}.

        Gated exactly as cache_profile is. For an idle card."""
        from elastic_gpu_scheduler_amd.agent import cotenancy

        return self._solo_profile(cotenancy.chase_profile, card, share, sizes, window)

    def _solo_profile(self, profile, card: int, share: int, sizes: Sequence[int],
                      window: Dict[str, Any]) -> Dict[str, Any]:
        """cache_profile's and chase_profile's common part: the gate, the
        scratch plan's mask for `share`, the sweep, the tenant's entry."""
        layout = self.mask_layouts().get(card)
        if not layout or not layout.get("interleaved"):
            return {"ok": False, "reason": "unsupported-layout"}
        try:
            plan = CardMaskPlan(int(layout["cus"]), int(layout["granule"]))
        except ValueError:
            return {"ok": False, "reason": "unsupported-layout"}
        grant = plan.allocate(0, int(share))
        if not plan.whole_granules(grant.mask):
            return {"ok": False, "reason": "unsupported-layout"}
        report = profile(card, grant.mask, list(sizes), **window)
        report["tenant"] = {"core": int(share), "mask": mask_hex(grant.mask),
                            "cus": grant.cus}
        return report


def _xcd_or_skipped(probe, device: int, slice_mib: int, chunk_kib: int):
    """xcd_bandwidth, with its refusal to allocate on a full card turned
    into a skipped sub-report (like hbm_pattern_test's) instead of failing
    the whole cycle."""
    try:
        return probe.xcd_bandwidth(device, slice_mib, 3, chunk_kib)
    except RuntimeError as exc:
        if "insufficient free device memory" not in str(exc):
            raise
        return {"skipped": "insufficient free memory"}


def health_summary(report: Dict[str, Any]) -> Dict[str, Any]:
    """One card's entry of the gpu-health annotation: the verdict and the
    figures behind it, without the raw mismatch records."""
    pattern = report.get("pattern") or {}
    xcd = report.get("xcd") or []
    return {
        "index": report["index"],
        "healthy": report["healthy"],
        "reasons": report["reasons"],
        "hbm_gbps": round(report.get("hbm_gbps", 0.0), 1),
        "xcd_gbps": {str(e["xcc"]): round(e["gbps"], 1)
                     for e in ([] if "skipped" in xcd else xcd)},
        "hbm_mismatches": (None if "skipped" in pattern
                           else list(pattern.get("mismatches", []))),
        "mfma_mismatches": sum(e.get("mismatched_elements", 0)
                               for e in report.get("mfma") or []),
        "ts": int(time.time()),
    }


def _uid_tag(uid: str) -> int:
    h = 1469598103934665603
    for ch in uid.encode():
        h ^= ch
        h = (h * 1099511628211) % (1 << 64)
    return h
