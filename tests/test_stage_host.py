"""CPU: the stage engines' shared skeleton (csrc/stage_host.hpp, stage_host.cpp) as
a stand-alone program under AddressSanitizer and UBSan, with the HIP runtime and
hc_phmm_init stubbed (tests/cpp/stage_host_main.cpp). Stage::ensure_init passes
HC_PHMM_FLAG_KEEP_MODE, and when the engine's init, hipSetDevice, the stream's
creation or the once-only setup fails it leaves no stream, no table and no
"ready" behind, so the next call starts over; release_all drops every registered
stage's stream and buffers (a stage without a stream too) and may run twice;
call_frame hands out a result only on success, frees it on an error and turns
std::bad_alloc into HC_PHMM_ENOMEM after draining the stream."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_stage_host_under_sanitizers(tmp_path):
    exe = tmp_path / "stage_host_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(ROCM, "include"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "stage_host_main.cpp"),
                    os.path.join(ROOT, "gatk-haplotypecaller-cpp17_amd", "csrc", "stage_host.cpp"), "-o", str(exe)],
                   check=True)
    p = subprocess.run([str(exe)], timeout=120, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert p.stdout.strip() == "ok"
