"""Node-agent entrypoint: discover MI355X inventory + xGMI topology and
publish them onto this Node object, then keep them fresh.

The reference ecosystem runs elastic-gpu-agent (NVML-based, separate repo)
for this role; here it is part of the same framework. Run as a DaemonSet on
GPU nodes (deploy/elastic-gpu-agent-amd.yaml):

    python -m elastic_gpu_scheduler_amd.cmd.agent_main --node $NODE_NAME

Publishes:
  elasticgpu.io/gpu-inventory   per-card {core, memory_bytes, name, arch}
  elasticgpu.io/xgmi-topology   hop matrix for locality-aware placement
and optionally runs the HBM health probe each cycle, publishing sick cards
as zero-capacity placeholders (list position always equals the physical card
index) so the scheduler stops placing pods on them. --self-test adds the deep
per-card self-test every Nth cycle and publishes its verdicts as
  elasticgpu.io/gpu-health      per-card {healthy, reasons, figures}
--cu-masks enforces gpu-core: every fractional container placed on this node
is granted a CU mask sized to its share, recorded on the pod as
  elasticgpu.io/cu-mask         per-container {card, mask, cus, shared}
--co-tenancy qualifies an idle node: per card, two tenants in separate
processes under disjoint masks, each one's rate alone and next to the other.
--co-tenancy-cache does the same for a tenant whose working set fits a cache,
--co-tenancy-chase for a tenant bound by the latency of dependent loads,
--co-tenancy-mfma for a tenant on the matrix cores, whose clock is the
chip's and follows no mask; --co-tenancy-mfma-form runs that tenant with the
FP8 or block-scaled MX instructions in place of the bf16 one, and
--co-tenancy-mfma-operands lds with its operands re-read from LDS every step.
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import sys
import time


def shares_arg(text: str):
    """"A,B": two gpu-core shares, each 1..100."""
    try:
        shares = tuple(int(x) for x in text.split(","))
    except ValueError:
        shares = ()
    if len(shares) != 2 or not all(1 <= s <= 100 for s in shares):
        raise argparse.ArgumentTypeError(
            f"expected two shares of 1..100 as A,B, got {text!r}")
    return shares


def mib_list_arg(text: str):
    """"M[,M...]": working-set sizes in MiB, each 1..1024."""
    try:
        sizes = tuple(int(x) for x in text.split(","))
    except ValueError:
        sizes = ()
    if not sizes or not all(1 <= m <= 1024 for m in sizes):
        raise argparse.ArgumentTypeError(
            f"expected sizes of 1..1024 MiB as M[,M...], got {text!r}")
    return sizes


def mfma_forms_arg(text: str):
    """"FORM[,FORM...]": forms of the mfma tenant's instruction."""
    from elastic_gpu_scheduler_amd.agent.cotenancy import MFMA_FORMS

    forms = tuple(text.split(","))
    if not all(f in MFMA_FORMS for f in forms):
        raise argparse.ArgumentTypeError(
            f"expected forms out of {', '.join(MFMA_FORMS)} as FORM[,FORM...], "
            f"got {text!r}")
    return forms


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="elastic-gpu-agent-amd", description=__doc__)
    p.add_argument("--node", default=os.environ.get("NODE_NAME", ""),
                   help="node object to annotate (default: $NODE_NAME)")
    p.add_argument("--interval", type=float, default=300.0,
                   help="republish interval seconds (0 = publish once and exit)")
    p.add_argument("--health-check", action="store_true",
                   help="run the HBM bandwidth probe each cycle and exclude "
                        "unhealthy cards from the inventory")
    p.add_argument("--self-test", action="store_true",
                   help="gate on the deep self-test (HBM pattern, per-XCD "
                        "bandwidth, MFMA check) as well; implies --health-check")
    p.add_argument("--self-test-every", type=int, default=12, metavar="N",
                   help="with --self-test: run the deep test on the first "
                        "cycle and every Nth after, the plain health check in "
                        "between (a deep run allocates about 1 GiB per card "
                        "and saturates it for a moment)")
    p.add_argument("--cu-masks", action="store_true",
                   help="enforce gpu-core: each cycle grant a CU mask to every "
                        "fractional container placed on this node and record "
                        "it as the pod's elasticgpu.io/cu-mask annotation")
    p.add_argument("--cu-mask-layout", action="store_true",
                   help="measure how CU-mask bits map to XCDs on each card, "
                        "print it as JSON and exit")
    p.add_argument("--co-tenancy", nargs="?", type=shares_arg, const=(50, 50),
                   default=None, metavar="A,B",
                   help="on each card in turn, run two tenants holding A and B "
                        "percent (default 50,50) as separate processes under "
                        "disjoint CU masks and print each one's FMA and HBM "
                        "stream rate alone and contended as JSON, then exit. "
                        "For an idle node: it saturates each card for about a "
                        "second per pair")
    p.add_argument("--co-tenancy-cache", nargs="?", type=mib_list_arg,
                   const=(12, 128), default=None, metavar="MIB[,MIB...]",
                   help="with --co-tenancy: instead of the FMA and stream "
                        "pairs, run a tenant that re-reads a working set of "
                        "each size (default 12,128 MiB) next to another such "
                        "tenant, next to the 1 GiB streamer (both ways round) "
                        "and next to an FMA tenant, and print one report per "
                        "card and size")
    p.add_argument("--co-tenancy-chase", nargs="?", type=mib_list_arg,
                   const=(2, 64, 1024), default=None, metavar="MIB[,MIB...]",
                   help="with --co-tenancy: instead of the FMA and stream "
                        "pairs, run a tenant that follows a chain of "
                        "dependent loads through a working set of each size "
                        "(default 2,64,1024 MiB: inside one XCD's L2, inside "
                        "the Infinity Cache, in HBM) next to another such "
                        "tenant, next to the 1 GiB streamer (both ways round) "
                        "and next to an FMA tenant, and print one report per "
                        "card and size; not together with --co-tenancy-cache")
    p.add_argument("--co-tenancy-mfma", action="store_true",
                   help="with --co-tenancy: instead of the FMA and stream "
                        "pairs, run a tenant that issues bf16 MFMAs back to "
                        "back from registers next to another such tenant, "
                        "next to the 1 GiB streamer (both ways round) and "
                        "next to an FMA tenant, and print one report per "
                        "card: each ratio with the part of it that the shader "
                        "clock explains (clock_ratio) and the part that it "
                        "does not (cycle_ratio); not together with "
                        "--co-tenancy-cache or --co-tenancy-chase")
    p.add_argument("--co-tenancy-mfma-form", type=mfma_forms_arg, default=None,
                   metavar="FORM[,FORM...]",
                   help="with --co-tenancy-mfma: the instruction the MFMA "
                        "tenants issue, out of bf16, fp8 (e4m3, the bf16 "
                        "rate), mxfp8 and mxfp4 (block-scaled, 2 x and 4 x "
                        "the bf16 work per clock); one report per card and "
                        "form, one after another")
    p.add_argument("--co-tenancy-mfma-operands", choices=("registers", "lds"),
                   default=None,
                   help="with --co-tenancy-mfma: where the MFMA tenants take "
                        "their operands from: registers (what they do when "
                        "the flag is absent), or lds, re-read from LDS before "
                        "every step as a GEMM or attention kernel re-reads "
                        "its own; combines with --co-tenancy-mfma-form")
    p.add_argument("--source", default="auto",
                   choices=("auto", "gpuprobe", "amdsmi", "amd-smi",
                            "rocm-smi", "torch"))
    p.add_argument("--dry-run", action="store_true",
                   help="print the annotations instead of patching the node")
    p.add_argument("--log-level", default="info")
    return p


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    logging.basicConfig(
        level=getattr(logging, args.log_level.upper(), logging.INFO),
        format="%(asctime)s %(levelname)s %(name)s %(message)s")
    log = logging.getLogger("egs.agent.main")

    from elastic_gpu_scheduler_amd.agent.agent import NodeAgent

    if args.cu_mask_layout:
        agent = NodeAgent(args.node or "local", client=None,
                          prefer_source=args.source)
        print(json.dumps(agent.mask_layouts(), indent=2))
        return 0

    def given(flag: str) -> bool:
        return getattr(args, flag[2:].replace("-", "_")) not in (None, False)

    # A flag, the flag it needs, and the flags whose runs are separate from its.
    for flag, needs, apart in (
            ("--co-tenancy-cache", "--co-tenancy", ()),
            ("--co-tenancy-chase", "--co-tenancy", ("--co-tenancy-cache",)),
            ("--co-tenancy-mfma", "--co-tenancy",
             ("--co-tenancy-cache", "--co-tenancy-chase")),
            ("--co-tenancy-mfma-form", "--co-tenancy-mfma", ()),
            ("--co-tenancy-mfma-operands", "--co-tenancy-mfma", ())):
        if not given(flag):
            continue
        if not given(needs):
            print(f"{flag} needs {needs}", file=sys.stderr)
            return 2
        for other in apart:
            if given(other):
                print(f"{flag} and {other} are separate runs", file=sys.stderr)
                return 2

    if args.co_tenancy is not None:
        from elastic_gpu_scheduler_amd.agent.cotenancy import (
            CACHE_PAIRS, CHASE_PAIRS, MFMA_PAIRS, cache_passes)

        # What every report of the run is asked for and, where a flag names
        # several forms or sizes, what each of them adds, by its label.
        common, each = {}, None
        if args.co_tenancy_mfma:
            common = {"pairs": MFMA_PAIRS}
            if args.co_tenancy_mfma_operands is not None:
                common["operands"] = args.co_tenancy_mfma_operands
            if args.co_tenancy_mfma_form is not None:
                each = {form: {"form": form} for form in args.co_tenancy_mfma_form}
        elif args.co_tenancy_chase is not None:
            common = {"pairs": CHASE_PAIRS}
            each = {str(mib): {"windows": {"chase": {"bytes": mib << 20}}}
                    for mib in args.co_tenancy_chase}
        elif args.co_tenancy_cache is not None:
            # A cache launch is given the bytes of a default stream launch, so
            # that neither tenant of a pair outlasts the other by far.
            common = {"pairs": CACHE_PAIRS}
            each = {str(mib): {"windows": {"cache": {
                "bytes": mib << 20, "passes": cache_passes(mib << 20)}}}
                for mib in args.co_tenancy_cache}
        agent = NodeAgent(args.node or "local", client=None,
                          prefer_source=args.source)

        def report(card, more):
            return agent.verify_isolation(card, args.co_tenancy, **common, **more)

        # One card, and one form or size, after another: never more than two
        # children at once.
        print(json.dumps({card: report(card, {}) if each is None else {
            label: report(card, more) for label, more in each.items()}
            for card in sorted(agent.mask_layouts())}, indent=2))
        return 0

    if args.dry_run:
        agent = NodeAgent(args.node or "dry-run-node", client=None,
                          prefer_source=args.source)
        print(json.dumps(agent.annotations(), indent=2))
        return 0

    if not args.node:
        print("--node (or $NODE_NAME) is required", file=sys.stderr)
        return 2

    from elastic_gpu_scheduler_amd.k8s.client import RealKubeClient

    client = RealKubeClient.from_env()
    agent = NodeAgent(args.node, client, prefer_source=args.source)

    cycle = 0
    while True:
        try:
            if args.self_test and cycle % max(args.self_test_every, 1) == 0:
                out = agent.publish_with_health(deep=True)
                if out["sick"]:
                    log.warning("self-test failed (published zero-capacity): %s",
                                out["sick"])
            elif args.health_check or args.self_test:
                out = agent.publish_with_health()
                if out["sick"]:
                    log.warning("unhealthy cards (published zero-capacity): %s",
                                out["sick"])
            else:
                agent.publish()
            log.info("published inventory for %s", args.node)
        except Exception:
            log.exception("publish failed; retrying next cycle")
        if args.cu_masks:
            try:
                masks = agent.sync_masks()
                log.info("cu masks held by %d pods", len(masks))
            except Exception:
                log.exception("cu-mask sync failed; retrying next cycle")
        cycle += 1
        if args.interval <= 0:
            return 0
        time.sleep(args.interval)


if __name__ == "__main__":
    sys.exit(main())
