"""CPU: the flat call's host record passes (csrc/flat_records.hpp: scan_pass,
fold_minis, fill_chunk and the packers) as a stand-alone program under
AddressSanitizer and UBSan (tests/cpp/flat_records_main.cpp). The caller's pools,
the output block and the descriptor array are heap blocks of exactly the bytes
the pairs use and pass 1 counted, so pass 2 writing anything but those bytes, or
either pass reading past a pool (the AVX2 paths' overlapping last 32 bytes), is an
error: one pair of R = H = 1; 513 pairs (one past a mini-task) cycling R and H
over the lengths either side of the 4-, 32- and 64-byte steps, from pair 0 and
from pair 7 of the pools, as one chunk and as two; an 'N' in a read, in a hap, a
quality below 33 and gap qualities that vary in a read's last byte, alone and
together, refused without scanning and packed like the scalar packers with it.
Also res_layout's offsets and RunEvents (engine_core.hpp) with stubbed HIP
events: a slot part run three times destroys the two triples it made and none
of its slot's."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_flat_records_under_sanitizers(tmp_path):
    exe = tmp_path / "flat_records_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(ROCM, "include"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-pthread", os.path.join(ROOT, "tests", "cpp", "flat_records_main.cpp"), "-o", str(exe)],
                   check=True)
    p = subprocess.run([str(exe)], timeout=120, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert p.stdout.strip() == "ok"
