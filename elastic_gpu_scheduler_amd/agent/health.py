"""Card health verdict from a deep self-test report.

`evaluate_card` is a pure function: no GPU, no I/O. The agent builds the
report (agent.NodeAgent.self_test) from the HIP probes' raw output and this
module turns it into {"healthy": bool, "reasons": [...]}.

Reasons:
  hbm-bandwidth      streaming-copy bandwidth below `limits.hbm_gbps`
  hbm-data           the pattern test read back a word it did not write
  mfma               a matrix-core result differed from the vector ALU's
  xcd-slow:<id>      that XCD read slower than `limits.xcd_ratio` x the
                     median of the card's XCDs (needs >= 3 XCDs reporting)
  xcd-checksum:<id>  that XCD's slice did not XOR to the expected pattern
  xcd-chunks:<id>    that XCD's slice was not read chunk-for-chunk once

A sub-report that was skipped ({"skipped": "..."}) is never a reason: a card
too full to test is not thereby a bad card.
"""
from __future__ import annotations

import statistics
from dataclasses import dataclass
from typing import Any, Dict, List


@dataclass(frozen=True)
class HealthLimits:
    hbm_gbps: float = 1000.0
    xcd_ratio: float = 0.5
    xcd_min_count: int = 3


def _skipped(sub: Any) -> bool:
    return sub is None or (isinstance(sub, dict) and "skipped" in sub)


def evaluate_card(report: Dict[str, Any],
                  limits: HealthLimits = HealthLimits()) -> Dict[str, Any]:
    reasons: List[str] = []

    bw = report.get("hbm_gbps")
    if bw is not None and bw < limits.hbm_gbps:
        reasons.append("hbm-bandwidth")

    pattern = report.get("pattern")
    if not _skipped(pattern) and any(pattern.get("mismatches", [])):
        reasons.append("hbm-data")

    mfma = report.get("mfma")
    if not _skipped(mfma) and any(e.get("mismatched_elements", 0) for e in mfma):
        reasons.append("mfma")

    xcd = report.get("xcd")
    if not _skipped(xcd):
        entries = sorted(xcd, key=lambda e: e["xcc"])
        if len(entries) >= limits.xcd_min_count:
            floor = limits.xcd_ratio * statistics.median(e["gbps"] for e in entries)
            reasons += [f"xcd-slow:{e['xcc']}" for e in entries
                        if e["gbps"] < floor]
        for e in entries:
            if ("expected_checksum" in e
                    and e["checksum"] != e["expected_checksum"]) \
                    or e.get("stable") is False:
                reasons.append(f"xcd-checksum:{e['xcc']}")
        for e in entries:
            if "expected_chunks" in e and e["chunks"] != e["expected_chunks"]:
                reasons.append(f"xcd-chunks:{e['xcc']}")

    return {"healthy": not reasons, "reasons": reasons}
