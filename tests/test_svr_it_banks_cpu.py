"""CPU: the pitch of k_svr_dense's insert-factor table, checked where it is decided - common.h, host-compiled into the stand-alone program
tests/svr_it_banks.cpp.  For every tile of 1..28 positions x 1..9 capture sizes the program enumerates the LDS addresses a half-wavefront's lanes read the
insert factors from: 32 distinct bank pairs wherever a padded, conflict-free pitch was chosen; the tile's LDS within 160 KiB at whatever pitch was chosen; the
benchmark's shapes (27 and 25 positions x 9 sizes) padded to 33, the 28 x 5 tile at its odd fallback."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_insert_table_pitch_is_conflict_free_and_fits(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is what the host tools are built with"
    exe = str(tmp_path / "svr_it_banks")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "svr_it_banks.cpp")], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    m = re.match(r"(\d+) tiles padded conflict free, (\d+) at the odd fallback pitch, (\d+) unpadded; 0 failures", p.stdout.decode())
    assert m, p.stdout.decode()
    padded, fallback, plain = map(int, m.groups())
    assert padded + fallback + plain == 28 * 9 and padded > 200          # every tile was looked at; nearly all of them have the room for the padded pitch
