"""The deletion alleles of DESIGN 4.21 restated by brute force (test oracle for mipgen_accel_reads_consensus_deletions, the deletion helpers of gapped_align.h and
`mipgen_count -pileup FILE -pileup_indels W -pileup_deletions DEL`): gapped_ref.side_view per side, pileup_ref.vote per position, a scan for maximal runs of `del`
along the molecule, a dictionary of alleles.  No lanes, no ballot, no rounds; the 64-bit key is computed only to put the finished alleles in order.  Test
infrastructure."""
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests import gapped_ref as G
from tests import pileup_ref as PR

EXT, LIG = G.EXT, G.LIG
DEPTH, STARTS, RAGGED, DEL = 0, 1, 2, 3
RECORD_DTYPE = np.dtype([("pos", "<i8"), ("length", "<i4"), ("count", "<i4"), ("ragged", "<i4"), ("depth", "<i4")])
TOTAL_KEYS = ("groups", "used", "depth", "deleted_bases", "events", "ragged", "alleles", "gapped_sides")
FILE_HEADER = ">sample\tmip_key\tchr\tposition\tstrand\tlength\tdeleted\tragged\tcount\tdepth\tppm\n"


def key(x: int, l: int, ragged: bool) -> int:
    return x << 35 | l << 1 | int(ragged)


def molecule_classes(es: bytes, eq: bytes, ls: bytes, lq: bytes, M: bytes, W: int, min_quality: int):
    """(c, flank, gapped sides) of one used molecule: c[t] the voted class at template position t (0..3, G.DISCORDANT, G.DEL or None) and flank[t] whether the molecule
    is discordant at t with one of its two usable observations a deletion."""
    e_obs, _e_ins, e_gaps = G.side_view(es, eq, M, W, EXT)
    l_obs, _l_ins, l_gaps = G.side_view(ls, lq, M, W, LIG)
    c, flank = [], []
    for t in range(len(M)):
        ue, ul = G.usable(e_obs.get(t), min_quality), G.usable(l_obs.get(t), min_quality)
        v = PR.vote(ue, ul)
        c.append(v)
        flank.append(v == G.DISCORDANT and G.DEL in (ue, ul))
    return c, flank, (e_gaps > 0) + (l_gaps > 0)


def events(c: Sequence[Optional[int]], flank: Sequence[bool]) -> List[Tuple[int, int, bool]]:
    """The maximal runs of G.DEL in c as (a, l, ragged), ascending a."""
    L, out, t = len(c), [], 0
    while t < L:
        if c[t] != G.DEL:
            t += 1
            continue
        a = t
        while t < L and c[t] == G.DEL:
            t += 1
        out.append((a, t - a, (a > 0 and flank[a - 1]) or (t < L and flank[t])))
    return out


def deletions(groups, mol_seq: Sequence[bytes], n: int, row: int, min_family: int = 1, min_quality: int = 0, W: int = 8, per_molecule: Optional[list] = None):
    """(sites[sum(len M_p)][4] int32 - depth, starts, ragged, del -, the records as an array of RECORD_DTYPE in ascending key order, totals) of the groups (cell, tag,
    family, ext_seq, ext_qual, lig_seq, lig_qual) whose cell lies in `row`.  per_molecule (a list, optional) receives (probe, template length, events) of every
    used molecule."""
    assert len(mol_seq) == n and all(len(M) >= 1 for M in mol_seq) and 1 <= W <= 15
    pos_off = [sum(len(M) for M in mol_seq[:p]) for p in range(n)]
    sites = np.zeros((sum(len(M) for M in mol_seq), 4), dtype=np.int32)
    alleles: Dict[Tuple[int, int, bool], int] = {}
    totals = dict.fromkeys(TOTAL_KEYS, 0)
    for cell, _tag, family, es, eq, ls, lq in groups:
        if cell // n != row:
            continue
        totals["groups"] += 1
        if family < min_family:
            continue
        totals["used"] += 1
        p = cell % n
        M = mol_seq[p]
        c, flank, gapped = molecule_classes(es, eq, ls, lq, M, W, min_quality)
        totals["gapped_sides"] += gapped
        for t in range(len(M)):
            if c[t] is not None and c[t] != G.DISCORDANT:
                sites[pos_off[p] + t][DEPTH] += 1
            if c[t] == G.DEL:
                sites[pos_off[p] + t][DEL] += 1
        found = events(c, flank)
        if per_molecule is not None:
            per_molecule.append((p, len(M), found))
        for a, l, ragged in found:
            x = pos_off[p] + a
            sites[x][STARTS] += 1
            sites[x][RAGGED] += ragged
            totals["deleted_bases"] += l
            alleles[(x, l, ragged)] = alleles.get((x, l, ragged), 0) + 1
    ordered = sorted(alleles.items(), key=lambda a: key(*a[0]))
    records = np.zeros(len(ordered), dtype=RECORD_DTYPE)
    for k, ((x, l, ragged), count) in enumerate(ordered):
        records[k] = (x, l, count, int(ragged), int(sites[x][DEPTH]))
    totals.update(depth=int(sites[:, DEPTH].sum()), events=int(sites[:, STARTS].sum()), ragged=int(sites[:, RAGGED].sum()), alleles=len(ordered))
    return sites, records, totals


def check_invariants(counts, sites, records, totals, g_totals) -> None:
    """The six invariants of DESIGN 4.21 between a deletions result and the gapped table of the same arguments."""
    assert np.array_equal(sites[:, 3], counts[:, 5])
    assert np.array_equal(sites[:, 0], counts[:, 0:4].sum(1) + counts[:, 5])
    n_pos = len(sites)
    per_pos, rag_pos, cover = np.zeros(n_pos, dtype=np.int64), np.zeros(n_pos, dtype=np.int64), np.zeros(n_pos + 1, dtype=np.int64)
    rag = records["ragged"] == 1
    np.add.at(per_pos, records["pos"], records["count"])
    np.add.at(rag_pos, records["pos"][rag], records["count"][rag])
    assert np.array_equal(per_pos, sites[:, 1]) and np.array_equal(rag_pos, sites[:, 2])
    np.add.at(cover, records["pos"], records["count"])
    np.add.at(cover, records["pos"] + records["length"], -records["count"].astype(np.int64))
    assert np.array_equal(np.cumsum(cover)[:n_pos], counts[:, 5])
    assert np.array_equal(records["depth"], sites[records["pos"], 0]) and (records["depth"] >= records["count"]).all() and (records["count"] >= 1).all()
    assert totals["deleted_bases"] == int((records["length"].astype(np.int64) * records["count"]).sum()) == g_totals["deletions"]


# ---- what `mipgen_count ... -pileup_deletions DEL` writes ------------------------------------------------------------------------------------------------------
def record_line(fields: Sequence[bytes], a: int, l: int) -> Tuple[int, str, str]:
    """(position, strand, deleted) of a record at template positions [a, a + l) of the probe whose table row is `fields`: the position is the LOWEST genome coordinate
    of the deleted bases; the deleted bytes are the template's as the pileup sees them, upper-cased, reverse-complemented on a minus probe (only A C G T complement)."""
    M = (fields[6] + fields[13] + fields[10]).upper()
    deleted = M[a:a + l]
    if fields[17] == b"+":
        return int(fields[3]) + a, "+", deleted.decode()
    return int(fields[4]) - (a + l - 1), "-", G.revcomp(deleted).decode()


def deletions_file(groups, table_rows: Sequence[Sequence[bytes]], labels: Optional[Sequence[str]] = None, min_family: int = 1, min_quality: int = 0,
                   W: int = 8) -> Tuple[bytes, str]:
    """(the -pileup_deletions file, its stderr line): one line per record, in row order, then table row order, then record order."""
    n = len(table_rows)
    mol_seq = [(f[6] + f[13] + f[10]).upper() for f in table_rows]
    pos_off = [sum(len(M) for M in mol_seq[:p]) for p in range(n)]
    n_rows = 1 if labels is None else len(labels) + 1
    out = [FILE_HEADER]
    n_alleles = n_events = n_ragged = bases = 0
    for row in range(n_rows):
        _sites, records, totals = deletions(groups, mol_seq, n, row, min_family, min_quality, W)
        n_alleles += totals["alleles"]; n_events += totals["events"]; n_ragged += totals["ragged"]; bases += totals["deleted_bases"]
        sample = "*" if labels is None else labels[row] if row < len(labels) else "undetermined"
        for rec in records:                                             # (ascending key: ascending position, so table row order)
            x, l, count, depth = int(rec["pos"]), int(rec["length"]), int(rec["count"]), int(rec["depth"])
            p = max(k for k in range(n) if pos_off[k] <= x)
            f = table_rows[p]
            pos, strand, deleted = record_line(f, x - pos_off[p], l)
            out.append(f"{sample}\t{f[0].decode()}\t{f[2].decode()}\t{pos}\t{strand}\t{l}\t{deleted}\t{int(rec['ragged'])}\t{count}\t{depth}\t{count * 1000000 // depth}\n")
    line = f"mipgen_count: deletion alleles {n_alleles} events {n_events} ragged {n_ragged} deleted_bases {bases}\n"
    return "".join(out).encode(), line
