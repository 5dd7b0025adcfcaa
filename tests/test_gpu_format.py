"""GPU: the all_mips record text of kernels_format.hip (k_fmt_count, k_fmt_records<false/true>, fmt_g6.h) where the golden designs never go.  Scores are
PLANTED: after score_window + replay_condense the window's dense score buffer is overwritten in place (tests/helpers.py: plant_scores), so the emitted
mask stays that of the real scores and the formatter meets every double of tests/fmt_cases.py.  The expected text is the oracle's: the emitted candidates
walked in generation order (position, capture size, arm pair, plus then minus), each line po.design + po.print_details (C printf).  Every comparison is
exact equality of the whole text; the byte count returned must be the sum of the line lengths and the record count the mask's population.

Two places lie outside the oracle: its mip index is a C int, and its printf keeps the sign of a NaN where the device prints "-nan" for every NaN
(fmt_g6.h).  There the score column comes from fmt_cases.expected, the name column from Python's own %04d, the other 18 columns from an oracle line.
The host side of fmt_g6.h on the same values: tests/test_fmt_cpu.py."""
import ctypes as C
import faulthandler
import math
import re
from collections import namedtuple

import numpy as np
import pytest

from mipgen_amd import capi, synth
from oracle import pyoracle as po
from tests import fmt_cases as FC
from tests import helpers as H

pytestmark = pytest.mark.gpu

LOGISTIC = capi.SCORE_LOGISTIC
MIDDLE = H.middle_of("5,3")
MIDDLE_MAX = 95                                   # sizeof(FmtConst::middle) - 1 (kernels.h)
INT_MAX = 2 ** 31 - 1

Emit = namedtuple("Emit", "region idx pi ki a s cand")     # idx: dense index inside the window; cand: the oracle's candidate tuple


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test's device work runs under a time limit of its own: a stuck call ends the process with a traceback instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def genome():
    return H.golden_genome()


def _snp_table(genome, lo, hi, step=7):
    return {p: chr(genome[p - 1]).upper() + "T" for p in range(lo, hi, step)}


def _region(genome, params, bed_start, bed_end, label="fmt", flank=3, mask_record=0):
    """40-60 bp of the golden chromosome with SNPs every 7 bases and a masked stretch: records with and without the _SNP_a suffix, all three flags."""
    return capi.build_region(genome, "1", bed_start, bed_end, params, bwa_mode="hashed", label=label, flank=flank, mask_record=mask_record,
                             snp_tab=_snp_table(genome, bed_start - 200, bed_end + 200))


def _names(regions, null=()):
    """mipgen_record_names of a run of regions (a ctypes array; entries listed in `null` get NULL chr and label)."""
    arr = (capi.RecordNames * max(len(regions), 1))()
    keep = []
    for i, rd in enumerate(regions):
        c, l = rd.chrom.encode(), rd.label.encode()
        keep += [c, l]
        arr[i] = capi.RecordNames(None, None, rd.start - 1, rd.stop) if i in null else capi.RecordNames(c, l, rd.start - 1, rd.stop)
    arr._keep = keep
    return arr


def _walk(P, grids, first_region, n_regions, first_candidate, mask):
    """The emitted candidates of a window in the reference's generation order (mipgen.cpp:421-491), as tests/test_oracle_golden.py walks them: the dense
    layout is strand-major inside a (position, capture size) row block, the generation order takes plus then minus of each pair."""
    A = P.n_arm_pairs
    out = []
    for ri in range(first_region, first_region + n_regions):
        g = grids[ri]
        if g.count == 0:
            continue
        base = g.offset - first_candidate
        m = mask[base:base + g.count].reshape(g.n_pos, g.n_sizes, 2, A)
        for pi, ki, a, s in np.argwhere(m.transpose(0, 1, 3, 2)).tolist():
            idx = base + ((pi * g.n_sizes + ki) * 2 + s) * A + a
            size = P.max_capture_size - (g.first_size_index + ki) * P.capture_increment
            out.append(Emit(ri, idx, pi, ki, a, s, (0, g.first_pos + pi, size, P.arm_ext[a], P.arm_lig[a], s)))
    return out


def _oracle_line(P, regions, em, score, middle, index):
    rd = regions[em.region]
    skipped, d = po.design(P, rd, em.cand)
    assert not skipped, em
    plain_nan = score != score and math.copysign(1.0, score) > 0
    big = index > INT_MAX
    line = po.print_details(rd, em.s, d, 0.0 if plain_nan else score, middle, 1 if big else index)
    if plain_nan or big:
        cols = line.split(b"\t")
        assert len(cols) == 20
        if plain_nan:
            assert cols[1] == b"0"
            cols[1] = FC.expected(score)
        if big:
            head = rd.label.encode() + b"_0001"
            assert cols[19].startswith(head)
            cols[19] = rd.label.encode() + b"_%04d" % index + cols[19][len(head):]
        line = b"\t".join(cols)
    return line


def _oracle_lines(P, regions, walk, scores, middle, first_index):
    return [_oracle_line(P, regions, em, float(scores[em.idx]), middle, first_index + i + 1) for i, em in enumerate(walk)]


def _require_text(text, n_records, lines, walk, scores, mask, what):
    """Exact equality of the whole text; a difference is shown with the score as float.hex and both lines."""
    assert n_records == len(lines) == int(np.count_nonzero(mask)), (what, n_records, len(lines), int(np.count_nonzero(mask)))
    want = b"".join(lines)
    if text != want:
        got = text.split(b"\n")
        for i, line in enumerate(lines):
            g = got[i] + b"\n" if i < len(got) - 1 else (got[i] if i < len(got) else None)
            if g != line:
                v = float(scores[walk[i].idx])
                gs = g.split(b"\t")[1] if g is not None and g.count(b"\t") > 1 else None
                ws = line.split(b"\t")[1]
                raise AssertionError(f"{what}: record {i} differs, score {v.hex()} ({v!r}): device prints {gs!r}, oracle {ws!r}\n"
                                     f" device: {g!r}\n oracle: {line!r}\n bytes {len(text)} vs {len(want)}")
        raise AssertionError(f"{what}: {len(text)} bytes where the oracle has {len(want)}: {text[len(want):len(want) + 200]!r}")
    assert len(text) == sum(len(l) for l in lines)


class Window:
    """One batch of regions in one result window: scored (logistic: no model), replayed, its real scores / records / mask and the walk kept."""

    def __init__(self, P, regions, null=()):
        self.P, self.regions = P, regions
        self.acc = capi.Accel(P)
        self.grids = self.acc.upload(regions)
        assert self.acc.window_count() == 1
        self.acc.score_window(0, LOGISTIC)
        self.acc.replay_condense()
        self.scores, self.records = self.acc.download()
        _, _, self.mask = self.acc.download_replay()
        self.walk = _walk(P, self.grids, 0, len(regions), 0, self.mask)
        self.walk_idx = np.array([em.idx for em in self.walk], dtype=np.int64)
        self.names = _names(regions, null)
        self.scores.setflags(write=False)

    def plant(self, values=None):
        """`values`: one score per emitted candidate in generation order (None: the real scores back); returns the whole planted array."""
        planted = self.scores.copy()
        if values is not None:
            planted[self.walk_idx] = values
        H.plant_scores(self.acc, planted)
        return planted

    def format(self, middle=MIDDLE, first_index=0):
        return self.acc.format_all_mips_array(self.names, middle, first_index)

    def check(self, planted, middle=MIDDLE, first_index=0, what=""):
        text, n = self.format(middle, first_index)
        lines = _oracle_lines(self.P, self.regions, self.walk, planted, middle, first_index)
        _require_text(text, n, lines, self.walk, planted, self.mask, what)
        return text, lines

    def close(self):
        self.acc.close()


@pytest.fixture(scope="module")
def win(genome):
    """The small window of the crafted-score, index and middle tests: one region of 45 bp, the default arm pairs (A = 57: two rounds of the slot loop)."""
    faulthandler.dump_traceback_later(300, exit=True)
    P = capi.make_params(150, 160, score_method=LOGISTIC)
    w = Window(P, [_region(genome, P, 9000, 9045)])
    faulthandler.cancel_dump_traceback_later()
    yield w
    w.close()


MAX_ROUNDS = 4         # 38,358 crafted values over the >= 10,000 emitted candidates of the window


def test_crafted_scores(win):
    """Every value of fmt_cases.crafted() through the device's fmt_g6 (device frexp / rint / fmod / floor / fma): cycled over the emitted candidates in
    plant -> format rounds in the order of a seeded permutation, so that the lanes of one wave scan hold score texts of 1 to 13 bytes
    (the first row block of the first round is laid out to hold all thirteen lengths) and a record_length that disagrees with write_record would shift
    the rest of the window."""
    vals = FC.crafted()
    texts = FC.expected_all(vals)
    E = len(win.walk)
    assert E >= 10000
    by_len = {}
    for k, t in enumerate(texts):
        by_len.setdefault(len(t), k)
    assert sorted(by_len) == list(range(1, 14))
    ladder = np.array([by_len[n] for n in range(1, 14)] * 4)                      # 52 neighbouring lanes, lengths 1..13 four times over
    last = win.walk[len(ladder) - 1]
    assert (last.pi, last.ki) == (0, 0) and 2 * last.a + last.s < 64               # ... all in the first 64 slots of the first row block
    seq = np.concatenate([ladder, np.random.default_rng(20240611).permutation(len(vals))])
    rounds = -(-len(seq) // E)
    assert rounds <= MAX_ROUNDS, (len(vals), E)
    printed = np.zeros(len(vals), dtype=bool)
    for r in range(rounds):
        pick = seq[r * E:(r + 1) * E]
        if len(pick) < E:                                                         # the last round: filled up with values that an earlier round held already
            pick = np.concatenate([pick, seq[len(ladder):len(ladder) + E - len(pick)]])
        planted = win.plant(vals[pick])
        assert np.array_equal(planted[win.walk_idx].view(np.uint64), vals[pick].view(np.uint64))
        _, lines = win.check(planted, what=f"crafted round {r}")
        for line, k in zip(lines, pick.tolist()):                                 # the oracle's printf and fmt_cases agree on what was asked for
            assert line.split(b"\t", 2)[1] == texts[k], (float(vals[k]).hex(), line.split(b"\t", 2)[1], texts[k])
        printed[pick] = True
    assert printed.all()


def _name_column(line, label):
    """(everything before the number, the number, what follows it) of a record whose last column is <label>_<number>[_SNP_a]."""
    head, last = line.rsplit(b"\t", 1)
    m = re.fullmatch(re.escape(label) + rb"_(\d{4,})((?:_SNP_a)?\n)", last)
    assert m, last
    return head + b"\t" + label + b"_", m.group(1), m.group(2)


def _renumber(line, label, index):
    head, _, tail = _name_column(line, label)
    return head + b"%04d" % index + tail


@pytest.fixture(scope="module")
def base_text(win):
    """The window's text with its real scores and first_index 0, held against the oracle once."""
    faulthandler.dump_traceback_later(300, exit=True)
    planted = win.plant()
    text, lines = win.check(planted, what="real scores, first_index 0")
    faulthandler.cancel_dump_traceback_later()
    return text, lines


@pytest.mark.parametrize("first_index", [0, 990, 9990, 99990, 2 ** 31 - 5, 10 ** 12])
def test_index_digits(win, base_text, first_index):
    """mip_name carries the running index as %04d: four characters below 1000, the number's own digits above.  The text numbered on from first_index is
    the text numbered from 0 with only that number changed, also where the index leaves the C int (Python's own formatting there); the first four
    cross their power of ten between two neighbouring lanes of one wave scan."""
    _, lines0 = base_text
    n = len(lines0)
    crossing = {0: 1000, 990: 1000, 9990: 10 ** 4, 99990: 10 ** 5}.get(first_index)
    if crossing is not None:
        k = crossing - first_index - 1                                            # the record that gets the first longer number
        assert 1 <= k < n
        a, b = win.walk[k - 1], win.walk[k]
        assert (a.pi, a.ki) == (b.pi, b.ki) and (2 * a.a + a.s) // 64 == (2 * b.a + b.s) // 64, (a, b)
    win.plant()
    text, nrec = win.format(first_index=first_index)
    label = win.regions[0].label.encode()
    want = [_renumber(line, label, first_index + i + 1) for i, line in enumerate(lines0)]
    assert nrec == n
    if first_index + n <= INT_MAX:                                                # (the oracle itself, where its int holds the index)
        assert want == _oracle_lines(win.P, win.regions, win.walk, win.scores, MIDDLE, first_index)
    _require_text(text, nrec, want, win.walk, win.scores, win.mask, f"first_index {first_index}")
    if crossing is not None:
        assert _name_column(want[k - 1], label)[1] == b"%04d" % (crossing - 1) and _name_column(want[k], label)[1] == b"%d" % crossing


POOL = synth.arm_pairs_from_sums(range(36, 50))        # 126 pairs, sums 49 .. 36


@pytest.mark.parametrize("A", [1, 32, 33, None])
def test_arm_pair_counts(genome, A):
    """The generation slots of a row block (2 * A, lanes of one wavefront, 64 per round of the slot loop): one pair, exactly one round (2 * A == 64), one
    slot pair into a second round (A = 33), and the default list (A = 57).  Three capture sizes per position (max_mip_overlap lifts the static skip), so
    the row block -> (position, size) decode is exercised too.  Real scores."""
    pairs = None if A is None else POOL[:A]
    P = capi.make_params(150, 160, score_method=LOGISTIC, arm_pairs=pairs, max_mip_overlap=200)
    assert P.n_arm_pairs == (57 if A is None else A)
    w = Window(P, [_region(genome, P, 9000, 9045)])
    try:
        assert w.grids[0].n_sizes == 3 and w.grids[0].count == w.grids[0].n_pos * 3 * 2 * P.n_arm_pairs
        assert len(w.walk) > w.grids[0].n_pos                                     # (more than one record per position)
        m = w.mask.reshape(w.grids[0].n_pos, 3, 2, P.n_arm_pairs)
        if A == 33:
            assert m[:, :, :, 32].any()                                           # slots 64 and 65: the second round of the slot loop writes records
        if A == 32:
            assert m[:, :, 1, 31].any()                                           # slot 63: the last lane of the only round
        w.check(w.plant(), what=f"A = {P.n_arm_pairs}")
    finally:
        w.close()


def test_regions_of_one_window_and_windows_numbered_on(genome):
    """Three regions in one window, the middle one with a grid of zero positions (upload takes it: its stop lies before the first scan position), so
    that find_region meets two equal first row blocks; chromosome names and labels of different lengths, one mipgen_record_names with NULL chr and
    label; planted scores.  Against the oracle, and against the same batch cut into one window per region numbered on from each other."""
    P = capi.make_params(150, 160, score_method=LOGISTIC)
    r0 = _region(genome, P, 9000, 9045, label="alpha")
    r1 = capi.RegionData(9500, 9300, 9200, genome[9199:9400].upper(), chrom="7_gl000195_random", label="nothing_to_scan_here", start=9500, stop=9300)
    r2 = _region(genome, P, 12000, 12052, label="", mask_record=1)
    r0.chrom, r2.chrom = "1", ""
    regions = [r0, r1, r2]
    w = Window(P, regions, null={2})
    try:
        assert [g.n_pos for g in w.grids] == [w.grids[0].n_pos, 0, w.grids[2].n_pos] and w.grids[0].n_pos > 0 and w.grids[2].n_pos > 0
        assert {em.region for em in w.walk} == {0, 2}
        vals = FC.crafted()
        pick = np.random.default_rng(20240612).permutation(len(vals))[:len(w.walk)]
        assert len(pick) == len(w.walk)
        planted = w.plant(vals[pick])
        one, _ = w.check(planted, what="three regions, one window")
        n_one = len(w.walk)
    finally:
        w.close()
    acc = capi.Accel(P)
    try:
        acc.set_window_breaks([1, 2])
        grids = acc.upload(regions)
        assert acc.window_count() == 3
        text, first = b"", 0
        for wi_ in range(3):
            wi = acc.window_info(wi_)
            assert (wi["first_region"], wi["n_regions"]) == (wi_, 1) and wi["n_candidates"] == grids[wi_].count
            acc.score_window(wi_, LOGISTIC)
            acc.replay_condense()
            c0, n = wi["first_candidate"], wi["n_candidates"]
            if n:
                _, _, mask = acc.download_replay(window=wi_)
                assert np.array_equal(mask, w.mask[c0:c0 + n])
            H.plant_scores(acc, planted[c0:c0 + n], window=wi_)
            t, k = acc.format_all_mips_array(_names(regions[wi_:wi_ + 1], null={0} if wi_ == 2 else ()), MIDDLE, first)
            assert (n == 0) == (k == 0)
            text += t
            first += k
        assert first == n_one
        assert text == one
    finally:
        acc.close()


def test_middle_lengths(win):
    """universal_middle_mip_seq: empty, and the longest the formatter takes (FmtConst::middle less its terminator); one byte more is refused with
    MIPGEN_E_INVALID and leaves the window's earlier text downloadable."""
    planted = win.plant()
    win.check(planted, middle=b"", what="empty middle")
    longest = (b"ACGTN" * 19)[:MIDDLE_MAX]
    assert len(longest) == MIDDLE_MAX
    text, _ = win.check(planted, middle=longest, what="longest middle")
    with pytest.raises(capi.AccelError, match=r"error -1: middle sequence too long"):
        win.format(middle=longest + b"A")
    buf = C.create_string_buffer(len(text))
    win.acc._check(win.acc.lib.mipgen_accel_download_text(win.acc.h, buf, len(text)))
    assert buf.raw == text
