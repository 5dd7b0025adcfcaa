"""Inputs for the banded alignment of DESIGN 4.13 where a lane-parallel aligner goes wrong, from a seeded numpy generator: low-complexity templates (the path has
many equal-scoring choices), reads with several competing edits, free ends on either border, bytes outside A C G T, short and long sides next to each other.
One generator for both routes: (q, M, W, side) cases for the stand-alone host program (tests/test_gapped_cpu.py) and whole molecules for a read session on the
device (tests/test_gpu_gapped_shapes.py).  Also what the tests need to describe their own inputs from the oracle alone: which sides the exact shortcut leaves
for the dynamic program (`listed`) and which kinds of path a side shows (`path_kinds`).  Test infrastructure."""
from typing import List, Sequence, Set, Tuple

import numpy as np

from tests import gapped_ref as G

ARM = 16
EXT, LIG = G.EXT, G.LIG
ACGT = b"ACGT"
TEMPLATE_KINDS = ("two_letter", "tandem", "runs", "random")
SESSION_SEED, SESSION_LENGTHS = 523, (33, 63, 64, 65, 96, 97, 130, 200) * 6       # the session of the device's test of random edits: 48 probes
PATH_KINDS = ("two_gap_runs", "ends_on_last_row", "ends_on_last_column", "touches_band_edge", "preference_changes_path")


def random_bases(rng, n: int, alphabet: bytes = ACGT) -> bytes:
    return bytes(alphabet[int(x)] for x in rng.integers(0, len(alphabet), n))


# ---- templates ---------------------------------------------------------------------------------------------------------------------------------------------
def template(rng, L: int, kind: str) -> bytes:
    """L bases over A C G T of one kind: a two-letter alphabet, tandem repeats of period 1 to 6 (a new unit every 8 to 40 bases), runs of 1 to 8 equal bases,
    or plain random."""
    if kind == "two_letter":
        pair = rng.choice(4, 2, replace=False)
        return random_bases(rng, L, bytes(ACGT[int(x)] for x in pair))
    if kind == "tandem":
        out = b""
        while len(out) < L:
            unit = random_bases(rng, int(rng.integers(1, 7)))
            out += (unit * 40)[:int(rng.integers(8, 41))]
        return out[:L]
    if kind == "runs":
        out, last = b"", -1
        while len(out) < L:
            b = int(rng.choice([x for x in ACGT if x != last]))
            out += bytes([b]) * int(rng.integers(1, 9)); last = b
        return out[:L]
    assert kind == "random"
    return random_bases(rng, L)


def with_odd_bytes(rng, M: bytes, n: int) -> bytes:
    """M with n of its bases replaced by N or by their own lower case (bytes that score 0 against everything, themselves included)."""
    out = bytearray(M)
    for t in rng.choice(len(M), min(n, len(M)), replace=False):
        out[t] = ord("N") if rng.random() < 0.5 else out[t] | 0x20
    return bytes(out)


# ---- reads ---------------------------------------------------------------------------------------------------------------------------------------------------
def read_length(rng, L: int, W: int = 15) -> int:
    """ARM + 1 .. L + W + 12, from two modes: about 20 bases, or about the template and beyond."""
    if rng.random() < 0.4:
        return int(rng.integers(ARM + 1, ARM + 9))
    return int(np.clip(rng.integers(L - 14, L + W + 13), ARM + 1, L + W + 12))


def edit_size(rng) -> int:
    """An indel of 1 to 16 bases: short, or any size, or (one in four) as wide as the widest band or one base off it."""
    u = rng.random()
    return int(rng.integers(1, 4)) if u < 0.4 else int(rng.choice([14, 15, 15, 15, 16])) if u < 0.65 else int(rng.integers(1, 17))


def side_read(rng, clean: bytes, odd: bytes, side: int, n: int, keep: int, lower_too: bool = False) -> bytes:
    """One read of n bytes for a side: the template `clean` (over A C G T) or its reverse complement; where the template shown to the aligner (`odd`) holds N
    the read holds N too half of the time (and, with lower_too, the same lower-case byte), so that a == b there; then 0 to 4 indels of 1 to 16 bases and 4 %
    substitutions, a third of them N, all behind the first `keep` bytes; random bases beyond the template's end."""
    r_clean, r_odd = (clean, odd) if side == EXT else (G.revcomp(clean), G.revcomp(odd))
    q = bytearray(r_clean)
    for x in range(keep, len(q)):
        if r_odd[x] not in ACGT and (r_odd[x] == ord("N") or lower_too) and rng.random() < 0.5:
            q[x] = r_odd[x]
    for _ in range(int(rng.integers(0, 5))):
        if len(q) <= keep:
            break
        at, size = int(rng.integers(keep, len(q))), edit_size(rng)
        if rng.random() < 0.5:
            del q[at:at + size]
        else:
            q[at:at] = random_bases(rng, size)
    for x in range(keep, len(q)):
        if rng.random() < 0.04:
            q[x] = ord("N") if rng.random() < 1 / 3 else ACGT[int(rng.integers(0, 4))]
    q += random_bases(rng, max(n - len(q), 0))
    return bytes(q[:n])


# ---- (q, M, W, side) cases for the host program ----------------------------------------------------------------------------------------------------------------
def side_cases(seed: int, n: int, lengths: Sequence[int] = (17, 33, 40, 63, 64, 65, 96, 130, 160)) -> List[Tuple[bytes, bytes, int, int]]:
    """n cases: every template kind in turn, one template in four with odd bytes, W from 1, 2, 4, 8, 15, both sides; edits anywhere behind the first base."""
    rng = np.random.default_rng(seed)
    cases = []
    for k in range(n):
        L = int(rng.choice(lengths))
        clean = template(rng, L, TEMPLATE_KINDS[k % 4])
        odd = with_odd_bytes(rng, clean, int(rng.integers(1, 4))) if k % 4 == 1 or k % 7 == 0 else clean
        W, side = int(rng.choice([1, 2, 4, 8, 15])), int(rng.integers(0, 2))
        q = side_read(rng, clean, odd, side, read_length(rng, L, W), keep=1, lower_too=True)
        cases.append((q, odd, W, side))
    return cases


# ---- whole molecules for a read session --------------------------------------------------------------------------------------------------------------------
class Probe:
    """One probe of a session: its two clean arms, the template shown to the pileup (M: arm + core + arm, perhaps with odd bytes anywhere in it, the arms included)
    and its molecules as (extension read, ligation read, family)."""

    def __init__(self, arms, M, molecules):
        self.arms, self.M, self.molecules = arms, M, molecules


def distinct_arms(rng, n: int) -> List[Tuple[bytes, bytes]]:
    """n pairs of random 16-base arms, no arm twice."""
    seen, out = set(), []
    while len(out) < n:
        e, l = random_bases(rng, ARM), random_bases(rng, ARM)
        if e != l and e not in seen and l not in seen:
            seen |= {e, l}; out.append((e, l))
    return out


def probes(seed: int, lengths: Sequence[int], per_probe=(8, 13), odd_every: int = 5) -> List[Probe]:
    """A probe per entry of `lengths` (each >= 2 ARM + 1): template = extension arm + a low-complexity core + ligation arm; every odd_every-th template carries
    odd bytes.  Per probe 8 to 12 molecules, families of 1 and 2; both reads of a molecule keep their first ARM bases, so the pair is assigned."""
    rng = np.random.default_rng(seed)
    arms = distinct_arms(rng, len(lengths))
    out = []
    for p, L in enumerate(lengths):
        assert L >= 2 * ARM + 1
        e, l = arms[p]
        clean = e + template(rng, L - 2 * ARM, TEMPLATE_KINDS[p % 4]) + l
        odd = with_odd_bytes(rng, clean, int(rng.integers(1, 5))) if p % odd_every == odd_every - 1 else clean
        mols = []
        for k in range(int(rng.integers(*per_probe))):
            n_e, n_l = read_length(rng, L), read_length(rng, L)
            mols.append((side_read(rng, clean, odd, EXT, n_e, ARM), side_read(rng, clean, odd, LIG, n_l, ARM), 1 + (k % 3 == 2)))
        out.append(Probe((e, l), odd, mols))
    return out


# ---- what a test says about its own inputs, from the oracle alone --------------------------------------------------------------------------------------------
def listed(q: bytes, M: bytes, side: int) -> bool:
    """DESIGN 4.13, the exact shortcut restated: a side goes to the dynamic program unless its min(m, L) leading bytes all equal the template's and are A C G T."""
    r = M if side == EXT else G.revcomp(M)
    k = min(len(q), len(r))
    return len(q) > 0 and any(q[x] != r[x] or q[x] not in ACGT for x in range(k))


def path_kinds(q: bytes, M: bytes, W: int, side: int, want_preference: bool = True) -> Set[str]:
    """Which of PATH_KINDS the oracle's path of this side shows."""
    r = M if side == EXT else G.revcomp(M)
    ie, je, _h, path = G.align(q, r, W, side)
    kinds = set()
    runs = sum(1 for x, s in enumerate(path) if s != "M" and (x == 0 or path[x - 1] != s))
    if runs >= 2:
        kinds.add("two_gap_runs")
    if ie == len(q) and je < len(r):
        kinds.add("ends_on_last_row")
    if je == len(r) and ie < len(q):
        kinds.add("ends_on_last_column")
    i = j = 0
    for s in path:
        i += s in "MI"; j += s in "MD"
        if abs(i - j) == W:
            kinds.add("touches_band_edge")
            break
    if want_preference and G.align(q, r, W, 1 - side)[3] != path:
        kinds.add("preference_changes_path")
    return kinds
