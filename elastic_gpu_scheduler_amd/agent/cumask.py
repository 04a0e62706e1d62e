"""CU-mask planner: turns the gpu-core fractions placed on one card into
per-container CU masks (pure Python, no GPU).

A process started with ROC_GLOBAL_CU_MASK=<hex>, or a stream made with
hipExtStreamCreateWithCUMask, runs only on the CUs its mask names: bit i is
CU i. On a multi-XCD card the driver deals the bits round-robin over the
XCDs (the probe's cu_mask_layout measures this), and a queue must keep at
least one CU on every XCD. So the unit of allocation is the granule:
`granule` consecutive bits aligned to `granule`, one CU on every XCD. Any set
of whole granules is XCD-balanced. A 256-CU, 8-XCD card has 32 granules; a
single-XCD (CPX) partition has granules of one CU.

A grant never changes while its key is held: a running process cannot have
its mask changed, so releasing and allocating never moves another tenant.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Hashable, List, Mapping


@dataclass(frozen=True)
class MaskGrant:
    mask: int     # bit i = CU i
    cus: int      # popcount of mask
    shared: bool  # True when granted granules other tenants already held


def mask_hex(mask: int) -> str:
    """The 0x... spelling ROC_GLOBAL_CU_MASK takes."""
    if mask < 0:
        raise ValueError("a CU mask is not negative")
    return hex(mask)


def parse_mask_hex(text: str) -> int:
    s = text.strip().lower()
    if s.startswith("0x"):
        s = s[2:]
    if not s or any(ch not in "0123456789abcdef" for ch in s):
        raise ValueError(f"not a hex CU mask: {text!r}")
    return int(s, 16)


def popcount(mask: int) -> int:
    return bin(mask).count("1")


class CardMaskPlan:
    """The masks granted on one card."""

    def __init__(self, cus: int, granule: int) -> None:
        if granule < 1 or cus < granule or cus % granule:
            raise ValueError(f"{cus} CUs do not divide into granules of {granule}")
        self.cus = cus
        self.granule = granule
        self.granules = cus // granule
        self._holders: List[int] = [0] * self.granules  # tenants per granule
        self._grants: Dict[Hashable, MaskGrant] = {}

    @property
    def full_mask(self) -> int:
        return (1 << self.cus) - 1

    def _granule_mask(self, g: int) -> int:
        return ((1 << self.granule) - 1) << (g * self.granule)

    def _touched(self, mask: int) -> List[int]:
        return [g for g in range(self.granules) if mask & self._granule_mask(g)]

    def whole_granules(self, mask: int) -> bool:
        """True when `mask` is a non-empty union of whole granules: the only
        masks known to leave every XCD a CU."""
        if mask <= 0 or mask > self.full_mask:
            return False
        return all(mask & self._granule_mask(g) == self._granule_mask(g)
                   for g in self._touched(mask))

    def allocate(self, key: Hashable, core: int) -> MaskGrant:
        """Grant `core` percent of the card: max(1, core * granules // 100)
        granules, free ones first-fit from the lowest. When the free ones run
        out (the one-granule minimum lets many tiny tenants oversubscribe a
        card) the rest come from the granules held by the fewest tenants and
        the grant is marked shared. Never fails; a held key keeps its grant."""
        held = self._grants.get(key)
        if held is not None:
            return held
        want = min(self.granules, max(1, core * self.granules // 100))
        take = [g for g in range(self.granules) if self._holders[g] == 0][:want]
        shared = len(take) < want
        if shared:
            taken = set(take)
            rest = sorted((g for g in range(self.granules) if g not in taken),
                          key=lambda g: (self._holders[g], g))
            take += rest[:want - len(take)]
        mask = 0
        for g in take:
            self._holders[g] += 1
            mask |= self._granule_mask(g)
        grant = MaskGrant(mask=mask, cus=popcount(mask), shared=shared)
        self._grants[key] = grant
        return grant

    def release(self, key: Hashable) -> None:
        grant = self._grants.pop(key, None)
        if grant is None:
            return
        for g in self._touched(grant.mask):
            self._holders[g] -= 1

    def grants(self) -> Dict[Hashable, MaskGrant]:
        return dict(self._grants)

    def restore(self, grants: Mapping[Hashable, MaskGrant]) -> "CardMaskPlan":
        """Take recorded grants as they are, overlaps included: they belong
        to processes already running under them. Returns self."""
        for key, grant in grants.items():
            if key in self._grants:
                continue
            if grant.mask <= 0 or grant.mask > self.full_mask:
                raise ValueError(f"recorded mask {hex(grant.mask)} does not fit "
                                 f"{self.cus} CUs")
            self._grants[key] = MaskGrant(mask=grant.mask,
                                          cus=popcount(grant.mask),
                                          shared=bool(grant.shared))
            for g in self._touched(grant.mask):
                self._holders[g] += 1
        return self
