"""CPU: the planner's wave packing of one sorted segment (csrc/seg_pack.hpp
pack_segment, called by planner.cpp pack_seg_waves) as a stand-alone program
under AddressSanitizer and UBSan: tests/cpp/seg_pack_main.cpp packs 200 seeded
lists of 1 to 3 000 (BC, nb, R) records — lists of one entry, of nb = 64
only and of nb = 1 only among them — and checks that every entry is placed
exactly once, each wave holds one width on at most 64 lanes, runs its first
pair's steps, and that its row bounds cover it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seg_pack_under_sanitizers(tmp_path):
    exe = tmp_path / "seg_pack_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "seg_pack_main.cpp"),
                    "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], timeout=120, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert p.stdout.strip() == "ok"
