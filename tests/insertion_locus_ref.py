"""The fold of insertion alleles to genome loci of DESIGN 4.19 restated by plain dictionary loops (test oracle for mipgen_accel_locus_insertion_tables, the
mipgen_accel_reads_consensus_locus_insertion* calls and `mipgen_count -insertion_loci / -call_insertion_loci`): every plan entry asked which anchor row it pulls,
every record of that row turned into a string, reverse-complemented as a string on a minus source, and counted in a dictionary per locus.  No map, no pairs, no
sort but the final one by key.  The pool and the calls are tests/insertion_call_ref.py on the folded rows; the files are composed with tests/locus_ref.py.  Test
infrastructure."""
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests import call_ref as CR
from tests import gapped_ref as G
from tests import insertion_call_ref as IC
from tests import insertion_ref as I
from tests import locus_ref as LR

TOTAL_KEYS = ("loci", "span", "insertions", "ins_discordant", "ambiguous", "alleles", "folded", "dropped")
LOCI_HEADER = ">sample\tchr\tposition\tlength\tinserted\tcount\tspan\tppm\tprobes\n"
CALLS_HEADER = ">sample\tchr\tposition\tlength\tinserted\tdepth\talt_count\talt_ppm\tbg_alt\tbg_depth\tq\tprobes\n"


def pulled_row(x: int, flags: int) -> Optional[int]:
    """The anchor row the source (x, flags) pulls: x - 1 under bit 1, x with flags 0, none on a minus source without bit 1."""
    if flags & LR.INS_FROM_PREVIOUS:
        assert x >= 1
        return x - 1
    return x if flags == 0 else None


def fold(records: np.ndarray, anchors: np.ndarray, plan: Sequence[int], n_loci: int):
    """(locus records as an array of insertion_ref.RECORD_DTYPE in ascending key order, locus_anchors [n_loci][4] int32, totals dict)."""
    n_pos = len(plan)
    assert anchors.shape == (n_pos, 4)
    by_row: Dict[int, List[int]] = {}
    for i, r in enumerate(records):
        assert 0 <= int(r["pos"]) < n_pos
        by_row.setdefault(int(r["pos"]), []).append(i)
    locus_anchors = [[0, 0, 0, 0] for _ in range(n_loci)]
    alleles: Dict[Tuple[int, int, Optional[bytes]], int] = {}            # (locus, length, string or None if ambiguous) -> count
    pulled = [0] * len(records)
    folded = 0
    for x in range(n_pos):
        e = int(plan[x])
        if e < 0:
            assert e == -1
            continue
        l, flags = e >> 2, e & 3
        assert 0 <= l < n_loci
        a = pulled_row(x, flags)
        if a is None:
            continue
        for c in range(4):
            locus_anchors[l][c] += int(anchors[a][c])
        for i in by_row.get(a, ()):
            r = records[i]
            length = int(r["length"])
            if r["ambiguous"]:
                s = None
            else:
                s = I.unpack(int(r["bases"]), length)
                if flags & LR.MINUS:
                    s = G.revcomp(s)
            k = (l, length, s)
            alleles[k] = alleles.get(k, 0) + int(r["count"])
            pulled[i] += 1
            folded += 1
    ordered = sorted(alleles.items(), key=lambda a: I.key(a[0][0], a[0][1], a[0][2] is None, 0 if a[0][2] is None else I.pack(a[0][2])))
    out = np.zeros(len(ordered), dtype=I.RECORD_DTYPE)
    for k, ((l, length, s), count) in enumerate(ordered):
        assert count < 2 ** 31
        out[k] = (l, length, count, 0 if s is None else I.pack(s), int(s is None))
    assert all(0 <= v < 2 ** 31 for row in locus_anchors for v in row)
    la = np.array(locus_anchors, dtype=np.int32).reshape(n_loci, 4)
    totals = {"loci": int(la.any(axis=1).sum()), "span": int(la[:, 0].sum(dtype=np.int64)), "insertions": int(la[:, 1].sum(dtype=np.int64)),
              "ins_discordant": int(la[:, 2].sum(dtype=np.int64)), "ambiguous": int(la[:, 3].sum(dtype=np.int64)), "alleles": len(ordered), "folded": folded,
              "dropped": sum(p == 0 for p in pulled)}
    assert sum(int(r["count"]) for r in out) == sum(int(r["count"]) * p for r, p in zip(records, pulled))
    return out, la, totals


def check_invariants(locus_records: np.ndarray, locus_anchors: np.ndarray, merged: Optional[np.ndarray], records: np.ndarray, plan: Sequence[int]) -> None:
    """The five invariants of DESIGN 4.19 on one fold; merged: the 8-column locus table of the same row (None: the first two are not asked)."""
    n_loci = len(locus_anchors)
    if merged is not None:
        assert np.array_equal(locus_anchors[:, 1], merged[:, 6]) and np.array_equal(locus_anchors[:, 2], merged[:, 7])
    per_locus, amb = [0] * n_loci, [0] * n_loci
    for r in locus_records:
        per_locus[int(r["pos"])] += int(r["count"])
        amb[int(r["pos"])] += int(r["count"]) if r["ambiguous"] else 0
    assert per_locus == [int(v) for v in locus_anchors[:, 1]] and amb == [int(v) for v in locus_anchors[:, 3]]
    times = {}
    for x, e in enumerate(plan):
        a = pulled_row(x, int(e) & 3) if int(e) >= 0 else None
        if a is not None:
            times[a] = times.get(a, 0) + 1
    assert sum(per_locus) == sum(int(r["count"]) * times.get(int(r["pos"]), 0) for r in records)


def session_rows(groups, mol_seq: Sequence[bytes], n_rows: int, plan: Sequence[int], n_loci: int, min_family: int = 1, min_quality: int = 0, W: int = 8):
    """Per row of a session (probe anchors, probe records, locus records, locus_anchors, fold totals), through insertion_ref.insertions and fold."""
    out = []
    for row in range(n_rows):
        anchors, records, _t = I.insertions(groups, mol_seq, len(mol_seq), row, min_family, min_quality, W)
        out.append((anchors, records) + fold(records, anchors, plan, n_loci))
    return out


def call_rows(folded, barcodes: bool, p: Dict[str, int], score=CR.exact_phred):
    """[(totals, candidates)] per row from session_rows' result: insertion_call_ref on the folded rows."""
    return IC.call_session([IC.Row(la, lrec) for _a, _r, lrec, la, _t in folded], barcodes, p, score)


# ---- what `mipgen_count ... -insertion_loci ILOCI -call_insertion_loci ILCALLS` writes ------------------------------------------------------------------------
def _inserted(rec) -> str:
    l = int(rec["length"])
    return "N" * l if rec["ambiguous"] else I.unpack(int(rec["bases"]), l).decode()


def files(groups, table_rows, labels: Optional[Sequence[str]], p: Optional[Dict[str, int]], parts: str = "target", min_family: int = 1, min_quality: int = 0, W: int = 8):
    """(ILOCI, its stderr line, ILCALLS, its stderr line, candidates excluded by the band); the last three None without call parameters."""
    plan, loci, _ref, n_sources = LR.build_plan(table_rows, parts)
    mol_seq = [(f[6] + f[13] + f[10]).upper() for f in table_rows]
    n_rows = 1 if labels is None else len(labels) + 1
    folded = session_rows(groups, mol_seq, n_rows, plan, len(loci), min_family, min_quality, W)
    out = [LOCI_HEADER]
    sums = dict.fromkeys(("alleles", "insertions", "ambiguous", "span"), 0)
    for row, (_a, _r, lrec, la, t) in enumerate(folded):
        for k in sums:
            sums[k] += t[k]
        for rec in lrec:
            l = int(rec["pos"])
            chrom, position = loci[l]
            span, count = int(la[l][0]), int(rec["count"])
            out.append(f"{LR.sample_name(labels, row)}\t{chrom.decode()}\t{position}\t{int(rec['length'])}\t{_inserted(rec)}\t{count}\t{span}\t{count * 1000000 // span}\t"
                       f"{n_sources[l]}\n")
    line = f"mipgen_count: insertion loci {len(loci)} alleles {sums['alleles']} events {sums['insertions']} ambiguous {sums['ambiguous']} span {sums['span']}\n"
    if p is None:
        return "".join(out).encode(), line, None, None, None
    calls = [CALLS_HEADER]
    cs = {"calls": 0, "candidates": 0, "tested": 0, "too_deep": 0, "excluded": 0}
    for row, (totals, cands) in enumerate(call_rows(folded, labels is not None, p)):
        for k in cs:
            cs[k] += totals[k]
        for l, length, bases, depth, k, K_o, N_o, q, _reserved in IC.kept_calls(cands, p):
            chrom, position = loci[l]
            calls.append(f"{LR.sample_name(labels, row)}\t{chrom.decode()}\t{position}\t{length}\t{I.unpack(bases, length).decode()}\t{depth}\t{k}\t{k * CR.MILLION // depth}\t"
                         f"{K_o}\t{N_o}\t{q}\t{n_sources[l]}\n")
    cline = f"mipgen_count: insertion locus calls {cs['calls']} candidates {cs['candidates']} tested {cs['tested']} too_deep {cs['too_deep']}\n"
    return "".join(out).encode(), line, "".join(calls).encode(), cline, cs["excluded"]
