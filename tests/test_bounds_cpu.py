"""CPU: the bounds skips of mipgen.cpp:443-444 in the three forms the dense-grid kernels use (mipgen_amd/csrc/mip_bounds.h) against the rule in the
reference's own words.  The header is host-compiled into the stand-alone program tests/bounds_host.cpp (g++, under the address and undefined-behaviour
sanitizers), which walks the whole box e, l in 1..12, C in 1..40, p in -2..48, seq_stop in {30, 31, 45}: no case is left out."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = 3 * 12 * 12 * 40 * 51                      # seq_stop, e, l, C, p


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is what the host tools are built with"
    exe = str(tmp_path_factory.mktemp("bounds") / "bounds_host")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "bounds_host.cpp")], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    return {k: int(v) for k, v in (line.split() for line in p.stdout.decode().splitlines())}


def test_the_box_is_walked_whole_and_holds_the_cases_that_matter(counts):
    assert counts["cases"] == BOX
    assert 0 < counts["constructed"] < BOX
    assert counts["low_p"] == 3 * 12 * 12 * 40 * 3                                      # p in {-2, -1, 0}
    assert counts["small_C"] > 0 and counts["small_C_else_ok"] > 0                        # C <= e + l, also where no other clause skips the candidate


def test_the_literal_rule_is_the_references(counts):
    assert counts["bad_literal"] == 0


def test_the_lane_test_of_the_row_form_equals_the_literal_rule(counts):
    assert counts["bad_lane"] == 0


def test_the_span_form_equals_the_literal_rule_as_the_kernel_evaluates_it(counts):
    assert counts["span_cases"] == BOX * 3 * 8                                           # inc in {1, 2, 5}, ki in 0..7
    assert counts["bad_span"] == 0


def test_the_uniform_test_of_the_row_form_never_says_all_where_a_pair_is_skipped(counts):
    n_lists = sum(2 * (a_hi - a_lo) + 1 for a_lo in range(1, 13) for a_hi in range(a_lo, 13))       # every [a_lo, a_hi] of 1..12, every max_sum in 2 a_lo..2 a_hi
    assert counts["uniform_cases"] == n_lists * 3 * 40 * 51
    assert counts["uniform_all"] > 0 and counts["uniform_pairs"] > counts["uniform_all"]
    assert counts["bad_uniform"] == 0
