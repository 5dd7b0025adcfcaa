"""The sample model of DESIGN 4.10 restated by brute force (test oracle for mipgen_accel_reads_*_samples and `mipgen_count -barcodes`): the index of
every pair is compared against every barcode by plain loops - no hash, no neighbour table, no chunks - every probe comes through
reads_ref.assign_reads, and tag groups are Python sets keyed (row, probe).  Test infrastructure."""
import math
from typing import Dict, List, Sequence, Tuple

import numpy as np

from tests import reads_ref as R

NONE, AMBIGUOUS = -1, -2
MAX_BARCODE = 32


def check_barcodes(barcodes: Sequence[bytes]) -> int:
    """The barcode length J, or ValueError for a set the model refuses."""
    if len(barcodes) < 1:
        raise ValueError("no barcode")
    J = len(barcodes[0])
    if not 1 <= J <= MAX_BARCODE:
        raise ValueError("barcode length outside 1..32")
    for b in barcodes:
        if len(b) != J:
            raise ValueError("barcodes of unequal length")
        if not all(c in R.ACGT for c in b):
            raise ValueError("a barcode byte that is not upper-case A C G T")
    if len(set(barcodes)) != len(barcodes):
        raise ValueError("duplicate barcodes")
    return J


def hamming(index: bytes, barcode: bytes) -> int:
    """Over the positions of the barcode; a byte of the index that is not upper-case A C G T is a mismatch at its position."""
    d = 0
    for j in range(len(barcode)):
        if index[j] != barcode[j] or index[j] not in R.ACGT:
            d += 1
    return d


def sample_of(index: bytes, barcodes: Sequence[bytes], d: int) -> int:
    """Sample of one index read: the barcode at the smallest distance <= d; NONE if there is none (or the read is shorter than a barcode),
    AMBIGUOUS if two barcodes share that smallest distance."""
    J = len(barcodes[0])
    if len(index) < J:
        return NONE
    best, best_s, ties = d + 1, NONE, 0
    for s, b in enumerate(barcodes):
        h = hamming(index, b)
        if h < best:
            best, best_s, ties = h, s, 1
        elif h == best and h <= d:
            ties += 1
    return AMBIGUOUS if ties > 1 else best_s


def assign_samples(index_reads: Sequence[bytes], barcodes: Sequence[bytes], d: int = 0) -> np.ndarray:
    """sample_of for every index read: a plain loop over every barcode, the pairs of one barcode compared at once."""
    J = check_barcodes(barcodes)
    assert d in (0, 1)
    X = np.zeros((len(index_reads), J), dtype=np.uint8)                  # 0 where the read has ended: never a base
    long_enough = np.zeros(len(index_reads), dtype=bool)
    for i, r in enumerate(index_reads):
        t = r[:J]
        X[i, :len(t)] = np.frombuffer(t, dtype=np.uint8)
        long_enough[i] = len(r) >= J
    not_base = ~np.isin(X, np.frombuffer(b"ACGT", dtype=np.uint8))
    best = np.full(len(index_reads), d + 1, dtype=np.int64)
    best_s = np.full(len(index_reads), NONE, dtype=np.int64)
    ties = np.zeros(len(index_reads), dtype=np.int64)
    for s, b in enumerate(barcodes):
        h = ((X != np.frombuffer(b, dtype=np.uint8)[None, :]) | not_base).sum(axis=1)
        better = long_enough & (h < best)
        tie = long_enough & (h == best) & (h <= d)
        best[better] = h[better]; best_s[better] = s; ties[better] = 1
        ties[tie] += 1
    best_s[ties > 1] = AMBIGUOUS
    return best_s.astype(np.int32)


def min_pairwise_distance(barcodes: Sequence[bytes]) -> int:
    a = np.array([np.frombuffer(b, dtype=np.uint8) for b in barcodes])
    best = a.shape[1]
    for i in range(len(a) - 1):
        best = min(best, int((a[i + 1:] != a[i]).sum(axis=1).min()))
    return best


def count_reads_samples(arms, ext_reads, lig_reads, index_reads, barcodes, barcode_mismatches: int = 0, tag_sizes=(5, 0), mismatches: int = 0,
                        swap_reads: bool = False):
    """(reads[rows][n], unique_tags[rows][n], totals, row_pairs[rows], sample_index, probe_index) of the model; rows = samples + 1, the last row
    is `undetermined`.  totals: the six of reads_ref.count_reads over all pairs, and sample_none, sample_ambiguous."""
    if swap_reads:
        ext_reads, lig_reads = lig_reads, ext_reads
    assert len(ext_reads) == len(lig_reads) == len(index_reads)
    te, tl = tag_sizes
    n, n_samples = len(arms), len(barcodes)
    probe = R.assign_reads(arms, ext_reads, lig_reads, tag_sizes, mismatches)
    sample = assign_samples(index_reads, barcodes, barcode_mismatches)
    reads = np.zeros((n_samples + 1, n), dtype=np.int64)
    row_pairs = np.zeros(n_samples + 1, dtype=np.int64)
    groups: Dict[Tuple[int, int], set] = {}
    tag_n = 0
    for i in range(len(probe)):
        row = int(sample[i]) if sample[i] >= 0 else n_samples
        row_pairs[row] += 1
        p = int(probe[i])
        if p < 0:
            continue
        reads[row, p] += 1
        tag = ext_reads[i][:te] + lig_reads[i][:tl]
        if all(c in R.ACGT for c in tag):
            groups.setdefault((row, p), set()).add(tag)
        else:
            tag_n += 1
    if te + tl == 0:
        unique = reads.copy()
    else:
        unique = np.zeros_like(reads)
        for (row, p), g in groups.items():
            unique[row, p] = len(g)
    totals = {"pairs": len(probe), "assigned": int((probe >= 0).sum()), "ambiguous": int((probe == R.AMBIGUOUS).sum()),
              "unassigned": int((probe == R.UNASSIGNED).sum()), "tag_n": tag_n, "overflow": 0,
              "sample_none": int((sample == NONE).sum()), "sample_ambiguous": int((sample == AMBIGUOUS).sum())}
    return reads, unique, totals, row_pairs, sample, probe.astype(np.int32)


# ---- what `mipgen_count -barcodes` writes -------------------------------------------------------------------------------------------------------
def counts_tsv(labels: Sequence[str], keys_names: Sequence[Tuple[str, str]], reads: np.ndarray, unique: np.ndarray) -> bytes:
    """-o: one line per cell with reads > 0, samples in file order, `undetermined` last, probes in table order."""
    out = ["sample\tmip_key\tmip_name\treads\tunique_tags"]
    for row, lab in enumerate(list(labels) + ["undetermined"]):
        for p, (k, nm) in enumerate(keys_names):
            if reads[row, p] > 0:
                out.append(f"{lab}\t{k}\t{nm}\t{int(reads[row, p])}\t{int(unique[row, p])}")
    return ("\n".join(out) + "\n").encode()


def samples_tsv(labels: Sequence[str], barcodes: Sequence[bytes], reads: np.ndarray, unique: np.ndarray, row_pairs: np.ndarray) -> bytes:
    """-samples: one line per sample, always; the last line is `undetermined` with barcode `*`."""
    out = ["sample\tbarcode\tpairs\tassigned\tunique_tags\tprobes_seen"]
    for row, (lab, bc) in enumerate(zip(list(labels) + ["undetermined"], [b.decode() for b in barcodes] + ["*"])):
        out.append(f"{lab}\t{bc}\t{int(row_pairs[row])}\t{int(reads[row].sum())}\t{int(unique[row].sum())}\t{int((reads[row] > 0).sum())}")
    return ("\n".join(out) + "\n").encode()


def labels_values(kind: str, reads: np.ndarray, unique: np.ndarray) -> List:
    """-labels: the value per probe over the NAMED samples (molecules of different samples are different molecules)."""
    r, u = reads[:-1].sum(axis=0), unique[:-1].sum(axis=0)
    if kind == "reads":
        return [int(v) for v in r]
    if kind == "tags":
        return [int(v) for v in u]
    return [math.log10(float(v) + 1.0) for v in u]


def stderr_lines(totals: Dict[str, int], n_samples: int) -> str:
    return (f"mipgen_count: pairs {totals['pairs']} assigned {totals['assigned']} ambiguous {totals['ambiguous']} unassigned {totals['unassigned']} "
            f"tag_n {totals['tag_n']} overflow {totals['overflow']}\n"
            f"mipgen_count: samples {n_samples} sample_none {totals['sample_none']} sample_ambiguous {totals['sample_ambiguous']}\n")
