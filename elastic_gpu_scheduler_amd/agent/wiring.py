"""From one pod's annotations to what its containers must be started with:
exactly what a kubelet device plugin's Allocate would return for them.

  * a whole-card container sees its cards (HIP_VISIBLE_DEVICES) and no mask;
  * a fractional container lives on one card and, when the agent granted it
    a CU mask (agent/cumask.py), is confined to its share of that card's CUs
    by ROC_GLOBAL_CU_MASK, which the HIP runtime applies to every queue the
    process creates.
"""
from __future__ import annotations

import json
from typing import Any, Dict, Mapping, Optional

from elastic_gpu_scheduler_amd.k8s import objects as obj
from elastic_gpu_scheduler_amd.utils import types as t

ENV_VISIBLE_DEVICES = "HIP_VISIBLE_DEVICES"
ENV_CU_MASK = "ROC_GLOBAL_CU_MASK"

MaskEntries = Dict[str, Dict[str, Any]]


def pod_cu_masks(pod: obj.Pod) -> MaskEntries:
    """The elasticgpu.io/cu-mask annotation, {container: {card, mask, cus,
    shared}}; {} when absent or malformed."""
    ann = (pod.get("metadata", {}) or {}).get("annotations", {}) or {}
    raw = ann.get(t.ANNOTATION_POD_CU_MASK)
    if not raw:
        return {}
    try:
        out: MaskEntries = {}
        for name, e in json.loads(raw).items():
            out[str(name)] = {"card": int(e["card"]), "mask": str(e["mask"]),
                              "cus": int(e["cus"]), "shared": bool(e["shared"])}
        return out
    except (ValueError, TypeError, KeyError, AttributeError):
        return {}


def fractional_core(container: Dict[str, Any]) -> int:
    """The gpu-core share a container must be held to, or 0: the allocator's
    own rule (core < 100 is a fraction of one card). A container that asks
    for memory only claims no compute share and gets no mask."""
    unit = obj.container_gpu_unit(container)
    if unit.gpu_count > 0 or unit.core >= t.GPU_CORE_EACH_CARD:
        return 0
    return max(int(unit.core), 0)


def container_wiring(pod: obj.Pod,
                     grants: Optional[Mapping[str, Mapping[str, Any]]] = None
                     ) -> Dict[str, Dict[str, Any]]:
    """{container: {"cards": [...], "env": {...}}} for the GPU containers of a
    placed pod. `grants` are the pod's mask entries (default: its cu-mask
    annotation). A pod without a complete placement yields {}."""
    allocation = obj.parse_allocation(pod)
    if allocation is None:
        return {}
    if grants is None:
        grants = pod_cu_masks(pod)
    out: Dict[str, Dict[str, Any]] = {}
    containers = pod.get("spec", {}).get("containers", []) or []
    for i, c in enumerate(containers):
        unit = obj.container_gpu_unit(c)
        if not unit.needs_gpu():
            continue
        cards = allocation[i]
        if not cards or (unit.gpu_count == 0 and len(cards) != 1):
            return {}
        name = c.get("name", str(i))
        env = {ENV_VISIBLE_DEVICES: ",".join(str(x) for x in cards)}
        grant = grants.get(name)
        if fractional_core(c) and grant and int(grant["card"]) == cards[0]:
            env[ENV_CU_MASK] = str(grant["mask"])
        out[name] = {"cards": list(cards), "env": env}
    return out
