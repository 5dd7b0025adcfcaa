"""The gapped pileup model of DESIGN 4.13 restated by brute force (test oracle for mipgen_accel_reads_consensus_pileup_gapped, the host functions of
gapped_align.h and `mipgen_count -pileup FILE -pileup_indels W`): per (molecule, side) the full (m + 1) x (L + 1) table with the band as a mask, a plain
traceback, then plain loops over groups and positions.  No shortcut, no lanes, no scan, no projection buffers.  Test infrastructure."""
import functools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests import pileup_ref as PR

NEG = -(10 ** 9)
ACGT = b"ACGT"
COLUMNS = ("A", "C", "G", "T", "discordant", "del", "ins", "ins_discordant")
DISCORDANT, DEL, INS, INS_DISCORDANT = 4, 5, 6, 7
EXT, LIG = 0, 1


def revcomp(seq: bytes) -> bytes:
    """Only A C G T complement; every other byte stays what it is."""
    return bytes(PR.COMPLEMENT.get(b, b) for b in reversed(seq))


def score(a: int, b: int) -> int:
    if a not in ACGT or b not in ACGT:
        return 0
    return 1 if a == b else -1


def table(q: bytes, r: bytes, W: int) -> List[List[int]]:
    """H over the whole (m + 1) x (L + 1) rectangle; NEG outside the band |i - j| <= W."""
    m, L = len(q), len(r)
    H = [[NEG] * (L + 1) for _ in range(m + 1)]
    H[0][0] = 0
    for i in range(m + 1):
        for j in range(max(0, i - W), min(L, i + W) + 1):        # (the cells the mask leaves; every other one stays NEG)
            if i == 0 and j == 0:
                continue
            best = NEG
            if i > 0 and j > 0 and H[i - 1][j - 1] > NEG:
                best = max(best, H[i - 1][j - 1] + score(q[i - 1], r[j - 1]))
            if j > 0 and H[i][j - 1] > NEG:
                best = max(best, H[i][j - 1] - 2)
            if i > 0 and H[i - 1][j] > NEG:
                best = max(best, H[i - 1][j] - 2)
            H[i][j] = best
    return H


def end_cell(H: List[List[int]], W: int) -> Tuple[int, int]:
    """Among the in-band cells of the last row or the last column: the largest H, then the smallest |j - i|, then the larger j (then the smaller i: the one tie
    the three leave open, two cells of the last column at equal distance above and below the diagonal)."""
    m, L = len(H) - 1, len(H[0]) - 1
    cells = [(i, j) for i in range(m + 1) for j in range(L + 1) if abs(i - j) <= W and (i == m or j == L)]
    return max(cells, key=lambda c: (H[c[0]][c[1]], -abs(c[1] - c[0]), c[1], -c[0]))


@functools.lru_cache(maxsize=None)
def align(q: bytes, r: bytes, W: int, side: int) -> Tuple[int, int, int, str]:
    """(end i, end j, score, path from (0, 0) to the end cell as 'M' / 'D' / 'I') of the query q against r."""
    H = table(q, r, W)
    ie, je = end_cell(H, W)
    i, j, steps = ie, je, []
    while i > 0 or j > 0:
        cand = {}
        if i > 0 and j > 0 and H[i - 1][j - 1] > NEG:
            cand["M"] = H[i - 1][j - 1] + score(q[i - 1], r[j - 1])
        if j > 0 and H[i][j - 1] > NEG:
            cand["D"] = H[i][j - 1] - 2
        if i > 0 and H[i - 1][j] > NEG:
            cand["I"] = H[i - 1][j] - 2
        step = next(s for s in ("MDI" if side == EXT else "DIM") if cand.get(s) == H[i][j])
        steps.append(step)
        if step in "MI":
            i -= 1
        if step in "MD":
            j -= 1
    return ie, je, H[ie][je], "".join(reversed(steps))


def side_view(q: bytes, qual: bytes, M: bytes, W: int, side: int):
    """What one side observes, in the orientation of M: ({t: (base byte or ord('-'), quality byte or None)}, {anchor t: insertion length} for the anchors the side
    covers, gap steps of its path).  A side of length 0 observes nothing."""
    L = len(M)
    if len(q) == 0:
        return {}, {}, 0
    r = M if side == EXT else revcomp(M)
    _ie, je, _h, path = align(q, r, W, side)
    t_of = (lambda j: j - 1) if side == EXT else (lambda j: L - j)      # column j (1-based) of r in M's orientation
    obs, ins_after, i, j = {}, {}, 0, 0
    for step in path:
        if step == "M":
            i += 1; j += 1
            base = q[i - 1]
            obs[t_of(j)] = (PR.COMPLEMENT.get(base, base) if side == LIG else base, qual[i - 1])
        elif step == "D":
            j += 1
            obs[t_of(j)] = (ord("-"), None)
        else:
            i += 1
            ins_after[j] = ins_after.get(j, 0) + 1                      # between column j and column j + 1 (j = 0: before the first column)
    assert j == je
    ins = {}
    for c in range(1, je):                                              # columns c and c + 1 are both consumed: the anchor is the lower of their positions
        ins[min(t_of(c), t_of(c + 1))] = ins_after.get(c, 0)
    return obs, ins, sum(1 for s in path if s != "M")


def usable(o, min_quality: int) -> Optional[int]:
    """The class of an observation - 0..3, DEL - or None."""
    if o is None:
        return None
    base, q = o
    if base == ord("-"):
        return DEL
    if base not in PR.COLUMN or q - 33 < min_quality:
        return None
    return PR.COLUMN[base]


def ins_vote(e: Optional[int], l: Optional[int]) -> Optional[int]:
    """e / l: the insertion length of a side that covers the anchor, None of one that does not."""
    if e is None and l is None:
        return None
    if e is None or l is None:
        one = l if e is None else e
        return INS if one > 0 else None
    if e != l:
        return INS_DISCORDANT
    return INS if e > 0 else None


def pileup(groups, mol_seq: Sequence[bytes], n: int, row: int, min_family: int = 1, min_quality: int = 0, W: int = 8) -> Tuple[np.ndarray, Dict[str, int]]:
    """(counts[sum(len M_p)][8] int32, totals) of the groups (cell, tag, family, ext_seq, ext_qual, lig_seq, lig_qual) whose cell lies in `row`."""
    assert len(mol_seq) == n and all(len(M) >= 1 for M in mol_seq) and 1 <= W <= 15
    pos_off = [sum(len(M) for M in mol_seq[:p]) for p in range(n)]
    counts = [[0] * 8 for _ in range(sum(len(M) for M in mol_seq))]
    totals = {"groups": 0, "used": 0, "gapped_sides": 0}
    for cell, _tag, family, es, eq, ls, lq in groups:
        if cell // n != row:
            continue
        totals["groups"] += 1
        if family < min_family:
            continue
        totals["used"] += 1
        p = cell % n
        M = mol_seq[p]
        e_obs, e_ins, e_gaps = side_view(es, eq, M, W, EXT)
        l_obs, l_ins, l_gaps = side_view(ls, lq, M, W, LIG)
        totals["gapped_sides"] += (e_gaps > 0) + (l_gaps > 0)
        for t in range(len(M)):
            v = PR.vote(usable(e_obs.get(t), min_quality), usable(l_obs.get(t), min_quality))       # (the vote of 4.12 with DEL as one more class)
            if v is not None:
                counts[pos_off[p] + t][v] += 1
            if t <= len(M) - 2:
                w = ins_vote(e_ins.get(t), l_ins.get(t))
                if w is not None:
                    counts[pos_off[p] + t][w] += 1
    c = np.array(counts, dtype=np.int32).reshape(-1, 8)
    totals.update(bases=int(c[:, :4].sum()), discordant=int(c[:, 4].sum()), deletions=int(c[:, 5].sum()), insertions=int(c[:, 6].sum()),
                  ins_discordant=int(c[:, 7].sum()))
    return c, totals


# ---- what `mipgen_count -pileup FILE -pileup_indels W` writes ---------------------------------------------------------------------------------------------
def line_counters(fields: Sequence[bytes], counts8, t: int) -> Tuple[int, str, str, str, List[int]]:
    """(position, strand, part, ref, the eight numbers of the line) of template position t of a probe whose table row is `fields` and whose counts are counts8
    [len M][8].  Bases as in 4.12; del stays at t; the insertion columns of the anchor between two bases go to the line of the LOWER genome coordinate of the
    two: anchor t on the plus strand, anchor t - 1 (between t - 1 and t) on the minus strand."""
    pos, strand, part, ref, acgt = PR.plus_strand(fields, t, counts8[t][:5])
    anchor = t if strand == "+" else t - 1
    ins = [int(counts8[anchor][6]), int(counts8[anchor][7])] if anchor >= 0 else [0, 0]
    return pos, strand, part, ref, acgt + [int(counts8[t][4]), int(counts8[t][5])] + ins


def pileup_file(groups, table_rows: Sequence[Sequence[bytes]], labels: Optional[Sequence[str]] = None, min_family: int = 1, min_quality: int = 0,
                W: int = 8) -> Tuple[bytes, str]:
    """(the -pileup file, the two stderr lines): one line per (row, probe, t) any of whose eight numbers is non-zero."""
    n = len(table_rows)
    mol_seq = [(f[6] + f[13] + f[10]).upper() for f in table_rows]
    n_rows = 1 if labels is None else len(labels) + 1
    out = [">sample\tmip_key\tchr\tposition\tstrand\tpart\tref\tA\tC\tG\tT\tdiscordant\tdel\tins\tins_discordant\n"]
    used = bases = nonref = disc = dels = ins = insd = gapped = 0
    for row in range(n_rows):
        counts, totals = pileup(groups, mol_seq, n, row, min_family, min_quality, W)
        used += totals["used"]; gapped += totals["gapped_sides"]
        sample = "*" if labels is None else labels[row] if row < len(labels) else "undetermined"
        at = 0
        for p, f in enumerate(table_rows):
            c8 = counts[at:at + len(mol_seq[p])]
            for t in range(len(mol_seq[p])):
                pos, strand, part, ref, k = line_counters(f, c8, t)
                if any(k):
                    out.append(f"{sample}\t{f[0].decode()}\t{f[2].decode()}\t{pos}\t{strand}\t{part}\t{ref}\t" + "\t".join(str(x) for x in k) + "\n")
                    bases += sum(k[:4]); disc += k[4]; dels += k[5]; ins += k[6]; insd += k[7]
                    nonref += sum(x for b, x in zip("ACGT", k[:4]) if b != ref)
            at += len(mol_seq[p])
    lines = (f"mipgen_count: pileup molecules {used} positions {len(out) - 1} bases {bases} nonref {nonref} discordant {disc}\n"
             f"mipgen_count: pileup indels deletions {dels} insertions {ins} ins_discordant {insd} gapped_sides {gapped}\n")
    return "".join(out).encode(), lines
