"""The locus model of DESIGN 4.15 restated by plain loops (test oracle for mipgen_accel_locus_tables, the mipgen_accel_reads_consensus_locus_* calls, the plan
builder of mipgen_amd/host/locus_plan.hpp and `mipgen_count -pileup_loci / -call_loci`): the plan from the rows of a MIP table, the fold of a count table per
template position into one row per genome locus, and the two files, composed with tests/call_ref.py.  Test infrastructure."""
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests import call_ref as CALL

MINUS, INS_FROM_PREVIOUS = 1, 2                     # the flag bits of a plan entry
COMPLEMENT = {65: 84, 67: 71, 71: 67, 84: 65}


class RefConflict(ValueError):
    """Two sources give one locus different refs: rows are 0-based table rows, first the earlier source."""
    def __init__(self, chrom, position, row_a, ref_a, row_b, ref_b):
        super().__init__(f"locus {chrom}:{position}: table row {row_a + 1} gives ref {chr(ref_a)}, table row {row_b + 1} gives ref {chr(ref_b)}")
        self.chrom, self.position, self.row_a, self.ref_a, self.row_b, self.ref_b = chrom, position, row_a, ref_a, row_b, ref_b


def sources_of(table_rows: Sequence[Sequence[bytes]], parts: str):
    """Every template position in table order as (x, included, chr, genome position, minus, t, plus-strand ref byte)."""
    assert parts in ("target", "all")
    x = 0
    for f in table_rows:
        E, T, L = f[6], f[13], f[10]
        M = (E + T + L).upper()
        minus = f[17] == b"-"
        for t in range(len(M)):
            included = parts == "all" or len(E) <= t < len(E) + len(T)
            position = int(f[4]) - t if minus else int(f[3]) + t
            ref = COMPLEMENT.get(M[t], M[t]) if minus else M[t]
            yield x, included, f[2], position, minus, t, ref
            x += 1


def build_plan(table_rows: Sequence[Sequence[bytes]], parts: str = "target"):
    """(plan - one int per template position -, loci - (chr, position) of every locus in locus order -, locus_ref bytes, sources per locus).  Loci: every
    (chr, position) an included template position lands on, chromosomes in order of first appearance in the table, then ascending position."""
    chrom_rank: Dict[bytes, int] = {}
    for f in table_rows:
        chrom_rank.setdefault(f[2], len(chrom_rank))
    row_of = []
    for i, f in enumerate(table_rows):
        row_of += [i] * (len(f[6]) + len(f[13]) + len(f[10]))
    first: Dict[Tuple[bytes, int], Tuple[int, int]] = {}          # locus -> (row, ref) of its first source
    for x, included, chrom, position, minus, t, ref in sources_of(table_rows, parts):
        if not included:
            continue
        key = (chrom, position)
        if key not in first:
            first[key] = (row_of[x], ref)
        elif first[key][1] != ref:
            raise RefConflict(chrom.decode(), position, first[key][0], first[key][1], row_of[x], ref)
    loci = sorted(first, key=lambda k: (chrom_rank[k[0]], k[1]))
    index = {k: l for l, k in enumerate(loci)}
    plan, n_sources = [], [0] * len(loci)
    for x, included, chrom, position, minus, t, ref in sources_of(table_rows, parts):
        if not included:
            plan.append(-1)
            continue
        l = index[(chrom, position)]
        n_sources[l] += 1
        plan.append(l * 4 + (MINUS if minus else 0) + (INS_FROM_PREVIOUS if minus and t >= 1 else 0))
    return plan, loci, bytes(first[k][1] for k in loci), n_sources


def merge(counts: np.ndarray, plan: Sequence[int], n_loci: int) -> np.ndarray:
    """The merged table [n_loci][columns] of counts [n_pos][columns] under the plan: Python integers, asserted to fit 32 bits."""
    n_pos, columns = counts.shape
    assert len(plan) == n_pos and columns in (5, 8)
    out = [[0] * columns for _ in range(n_loci)]
    for x in range(n_pos):
        e = int(plan[x])
        if e < 0:
            assert e == -1
            continue
        l, flags = e >> 2, e & 3
        assert 0 <= l < n_loci
        row = [int(v) for v in counts[x]]
        m = out[l]
        if flags & MINUS:
            m[0] += row[3]; m[1] += row[2]; m[2] += row[1]; m[3] += row[0]
        else:
            m[0] += row[0]; m[1] += row[1]; m[2] += row[2]; m[3] += row[3]
        m[4] += row[4]
        if columns == 8:
            m[5] += row[5]
            if flags & INS_FROM_PREVIOUS:
                assert x >= 1
                m[6] += int(counts[x - 1][6]); m[7] += int(counts[x - 1][7])
            elif not flags & MINUS:
                m[6] += row[6]; m[7] += row[7]
    assert all(0 <= v < 2 ** 31 for m in out for v in m)
    return np.array(out, dtype=np.int32).reshape(n_loci, columns)


def totals(merged: np.ndarray) -> Dict[str, int]:
    t = {"covered": 0, "bases": 0, "discordant": 0, "deletions": 0, "insertions": 0, "ins_discordant": 0}
    for row in merged:
        row = [int(v) for v in row]
        t["covered"] += any(row)
        t["bases"] += row[0] + row[1] + row[2] + row[3]
        t["discordant"] += row[4]
        if len(row) == 8:
            t["deletions"] += row[5]; t["insertions"] += row[6]; t["ins_discordant"] += row[7]
    return t


# ---- what `mipgen_count -pileup_loci / -call_loci` writes --------------------------------------------------------------------------------------------------
def sample_name(labels: Optional[Sequence[str]], row: int) -> str:
    return "*" if labels is None else labels[row] if row < len(labels) else "undetermined"


def loci_file(tables: Sequence[np.ndarray], table_rows, labels: Optional[Sequence[str]], parts: str = "target"):
    """(the -pileup_loci file, its stderr line) from the per-probe count table of EVERY row of the session."""
    plan, loci, ref, n_sources = build_plan(table_rows, parts)
    columns = tables[0].shape[1]
    out = [">sample\tchr\tposition\tref\tprobes\tA\tC\tG\tT\tdiscordant" + ("\tdel\tins\tins_discordant" if columns == 8 else "") + "\n"]
    lines = bases = nonref = disc = 0
    for row, counts in enumerate(tables):
        merged = merge(counts, plan, len(loci))
        for l, (chrom, position) in enumerate(loci):
            m = [int(v) for v in merged[l]]
            if not any(m):
                continue
            out.append(f"{sample_name(labels, row)}\t{chrom.decode()}\t{position}\t{chr(ref[l])}\t{n_sources[l]}\t" + "\t".join(str(v) for v in m) + "\n")
            lines += 1
            bases += sum(m[:4])
            nonref += sum(m[b] for b in range(4) if "ACGT"[b] != chr(ref[l]))
            disc += m[4]
    return "".join(out).encode(), f"mipgen_count: loci {len(loci)} lines {lines} bases {bases} nonref {nonref} discordant {disc}\n"


LOCUS_CALLS_HEADER = ">sample\tchr\tposition\tref\talt\tdepth\talt_count\talt_ppm\tbg_alt\tbg_depth\tq\tprobes\n"


def calls_file(tables: Sequence[np.ndarray], table_rows, labels: Optional[Sequence[str]], p: Dict[str, int], parts: str = "target"):
    """(the -call_loci file, its stderr line, candidates excluded by the band): DESIGN 4.14 with x := locus on the merged tables.  Lines: rows first, then locus
    order, then the alt classes A C G T - (the merged table is in plus orientation already)."""
    plan, loci, ref, n_sources = build_plan(table_rows, parts)
    merged = [merge(counts, plan, len(loci)) for counts in tables]
    n_sample = len(tables) - 1 if labels is not None else 1
    pool_ = CALL.pool(merged[:n_sample], p["bg_max_ppm"])
    out = [LOCUS_CALLS_HEADER]
    sums = {"calls": 0, "candidates": 0, "tested": 0, "too_deep": 0, "excluded": 0}
    for row, counts in enumerate(merged):
        tot, cands = CALL.call_cells(counts, pool_, ref, row < n_sample, p)
        for key in sums:
            sums[key] += tot[key]
        for l, a, n, k, K_o, N_o, q in CALL.kept_calls(cands, p):
            chrom, position = loci[l]
            out.append(f"{sample_name(labels, row)}\t{chrom.decode()}\t{position}\t{chr(ref[l])}\t{CALL.ALLELE_TEXT[a]}\t{n}\t{k}\t{k * CALL.MILLION // n}\t{K_o}\t{N_o}\t{q}\t"
                       f"{n_sources[l]}\n")
    stderr = f"mipgen_count: locus calls {sums['calls']} candidates {sums['candidates']} tested {sums['tested']} too_deep {sums['too_deep']}\n"
    return "".join(out).encode(), stderr, sums["excluded"]
