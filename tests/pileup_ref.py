"""The pileup model of DESIGN 4.12 restated by brute force (test oracle for mipgen_accel_reads_consensus_pileup and `mipgen_count -pileup`): a plain loop over
the groups that consensus_fetch or consensus_ref.consensus_reads lists, and inside it a plain loop over the template positions of the group's probe.  No cell
boundaries, no rounds, no lanes.  Test infrastructure."""
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

COLUMN = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
COMPLEMENT = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A")}
DISCORDANT = 4


def observation(seq: bytes, qual: bytes, at: int, complement: bool, min_quality: int) -> Optional[int]:
    """The column (0..3) of the usable observation a consensus read makes at its index `at`, or None: beyond the read, not one of A C G T (a ligation base is
    complemented first; anything else stays unusable), or below min_quality."""
    if at < 0 or at >= len(seq):
        return None
    base = seq[at]
    if complement:
        base = COMPLEMENT.get(base, base)
    if base not in COLUMN or qual[at] - 33 < min_quality:
        return None
    return COLUMN[base]


def vote(ext: Optional[int], lig: Optional[int]) -> Optional[int]:
    """One vote per molecule and position from its two observations: nothing, the one base, the shared base once, or `discordant` and no base."""
    if ext is None:
        return lig
    if lig is None or lig == ext:
        return ext
    return DISCORDANT


def pileup(groups, mol_len: Sequence[int], n: int, row: int, min_family: int = 1, min_quality: int = 0) -> Tuple[np.ndarray, Dict[str, int]]:
    """(counts[sum(mol_len)][5] int32, totals) of the groups (cell, tag, family, ext_seq, ext_qual, lig_seq, lig_qual) whose cell lies in `row`; cell = row * n +
    probe.  Probe p's positions start at sum(mol_len[:p]); position t of the extension consensus is base t of the molecule, position j of the ligation consensus
    the complement of base mol_len[p] - 1 - j; positions at or beyond mol_len[p] never come up, because t runs over the molecule only."""
    assert len(mol_len) == n and all(l >= 1 for l in mol_len)
    pos_off = [sum(mol_len[:p]) for p in range(n)]
    counts = [[0, 0, 0, 0, 0] for _ in range(sum(mol_len))]
    totals = {"groups": 0, "used": 0, "bases": 0, "discordant": 0}
    for cell, _tag, family, es, eq, ls, lq in groups:
        if cell // n != row:
            continue
        totals["groups"] += 1
        if family < min_family:
            continue
        totals["used"] += 1
        p = cell % n
        for t in range(mol_len[p]):
            v = vote(observation(es, eq, t, False, min_quality), observation(ls, lq, mol_len[p] - 1 - t, True, min_quality))
            if v is not None:
                counts[pos_off[p] + t][v] += 1
                totals["discordant" if v == DISCORDANT else "bases"] += 1
    return np.array(counts, dtype=np.int32).reshape(-1, 5), totals


# ---- the coordinate rule and what `mipgen_count -pileup` writes -----------------------------------------------------------------------------------------
def plus_strand(fields: Sequence[bytes], t: int, counts5: Sequence[int]) -> Tuple[int, str, str, str, List[int]]:
    """(position, strand, part, ref, [A, C, G, T]) in genome plus orientation of template position t of the table row `fields` (its 20 columns as bytes)."""
    E, T, L = fields[6], fields[13], fields[10]
    M = (E + T + L).upper()
    part = "ext" if t < len(E) else "target" if t < len(E) + len(T) else "lig"
    if fields[17] == b"+":
        return int(fields[3]) + t, "+", part, chr(M[t]), [int(c) for c in counts5[:4]]
    ref = COMPLEMENT.get(M[t], M[t])
    return int(fields[4]) - t, "-", part, chr(ref), [int(counts5[3]), int(counts5[2]), int(counts5[1]), int(counts5[0])]


def pileup_file(groups, table_rows: Sequence[Sequence[bytes]], labels: Optional[Sequence[str]] = None, min_family: int = 1, min_quality: int = 0) -> Tuple[bytes, str]:
    """(the -pileup file, the stderr line): one line per (row, probe, t) with a non-zero counter, rows first, then table order, then ascending t."""
    n = len(table_rows)
    mol_len = [len(f[6]) + len(f[13]) + len(f[10]) for f in table_rows]
    n_rows = 1 if labels is None else len(labels) + 1
    out = [">sample\tmip_key\tchr\tposition\tstrand\tpart\tref\tA\tC\tG\tT\tdiscordant\n"]
    used = bases = nonref = disc = 0
    for row in range(n_rows):
        counts, totals = pileup(groups, mol_len, n, row, min_family, min_quality)
        used += totals["used"]
        sample = "*" if labels is None else labels[row] if row < len(labels) else "undetermined"
        at = 0
        for p, f in enumerate(table_rows):
            for t in range(mol_len[p]):
                c = counts[at + t]
                if any(c):
                    pos, strand, part, ref, acgt = plus_strand(f, t, c)
                    out.append(f"{sample}\t{f[0].decode()}\t{f[2].decode()}\t{pos}\t{strand}\t{part}\t{ref}\t{acgt[0]}\t{acgt[1]}\t{acgt[2]}\t{acgt[3]}\t{int(c[4])}\n")
                    bases += sum(acgt); disc += int(c[4])
                    nonref += sum(k for b, k in zip("ACGT", acgt) if b != ref)
            at += mol_len[p]
    line = f"mipgen_count: pileup molecules {used} positions {len(out) - 1} bases {bases} nonref {nonref} discordant {disc}\n"
    return "".join(out).encode(), line
