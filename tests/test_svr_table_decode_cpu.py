"""CPU: the batch numbering of k_svr_dense's table stage and the integer side of its entries, checked where they are written - svr_table_decode.h,
host-compiled into the stand-alone program tests/svr_table_decode.cpp (under AddressSanitizer and UBSan).  For every tile of 1..28 positions x 1..9 capture
sizes and 29..90 positions x 1 size, both strands, the default arm pairs and a list with 3 extension and 2 ligation lengths, the program walks the work
counter's range lane by lane: every decoded LDS address and the slot a factor is stored to equal the formulas the kernel used before the batches were made
role-uniform; every upstream, downstream and insert entry is produced exactly once, idle lanes produce nothing; the LDS footprint is the restated sum."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_batches_decode_every_entry_once_at_the_old_addresses(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is what the host tools are built with"
    exe = str(tmp_path / "svr_table_decode")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "svr_table_decode.cpp")], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    m = re.match(r"(\d+) tile walks, (\d+) arm entries and (\d+) insert entries decoded, (\d+) idle lanes; 0 failures", p.stdout.decode())
    assert m, p.stdout.decode()
    walks, arm, ins, idle = map(int, m.groups())
    # 2 pair lists x 2 strands x (28 x 9 + 62) shapes, less the ones no tile has (more positions x sizes than lanes, or than LDS); both PF buffers walked
    assert 1000 < walks <= 2 * 2 * (28 * 9 + 62)
    assert arm > 10 ** 6 and ins > 5 * 10 ** 5 and idle > 0
