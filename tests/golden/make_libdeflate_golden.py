"""Writes tests/golden/libdeflate_members.npz: raw DEFLATE streams from a second
producer, libdeflate (which htslib uses for BAM), for the BGZF inflater's tests.

The system's libdeflate.so.0 is loaded through ctypes (libdeflate_alloc_compressor,
libdeflate_deflate_compress); the tests read the .npz only and never load it.
Inputs: bam_cases.libdeflate_inputs(), each at levels 1, 6, 9 and 12. The file
holds, as data:

    names        "<input>_level_<L>" per stream      streams, stream_off   the raw DEFLATE streams, end to end
    inputs       the inputs' names                   plain, plain_off      their bytes, end to end
    version      the library's version

    python tests/golden/make_libdeflate_golden.py [--version X.Y]
"""
import ctypes
import os
import re
import subprocess
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "gatk-haplotypecaller-cpp17_amd")]

import bam_cases as BC  # noqa: E402

LEVELS = (1, 6, 9, 12)


def version():
    if "--version" in sys.argv:
        return sys.argv[sys.argv.index("--version") + 1]
    try:
        with open("/usr/include/libdeflate.h") as f:
            m = re.search(r'LIBDEFLATE_VERSION_STRING\s+"([^"]+)"', f.read())
        if m:
            return m.group(1)
    except OSError:
        pass
    try:
        out = subprocess.run(["dpkg-query", "-W", "-f=${Version}", "libdeflate0"], capture_output=True, text=True).stdout
        if out:
            return out.strip()
    except OSError:
        pass
    return "unknown"


def main():
    lib = ctypes.CDLL("libdeflate.so.0")
    lib.libdeflate_alloc_compressor.restype = ctypes.c_void_p
    lib.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
    lib.libdeflate_deflate_compress.restype = ctypes.c_size_t
    lib.libdeflate_deflate_compress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    lib.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
    inputs = BC.libdeflate_inputs()
    names, streams = [], []
    for level in LEVELS:
        c = lib.libdeflate_alloc_compressor(level)
        assert c
        for name, data in inputs.items():
            room = ctypes.create_string_buffer(65536 - 26)          # what a BGZF member can hold
            n = lib.libdeflate_deflate_compress(c, data, len(data), room, len(room))
            assert n > 0, (name, level)
            assert zlib.decompress(room.raw[:n], -15) == data
            names.append(f"{name}_level_{level}")
            streams.append(room.raw[:n])
        lib.libdeflate_free_compressor(c)

    def ends(parts):
        return np.cumsum([0] + [len(p) for p in parts]).astype(np.int64)
    plain = list(inputs.values())
    out = os.path.join(HERE, "libdeflate_members.npz")
    np.savez_compressed(out, names=np.array(names, "S"), streams=np.frombuffer(b"".join(streams), np.uint8), stream_off=ends(streams),
                        inputs=np.array(list(inputs), "S"), plain=np.frombuffer(b"".join(plain), np.uint8), plain_off=ends(plain),
                        version=np.array(version(), "S"))
    print(f"{out}: {len(names)} streams, {sum(map(len, streams))} bytes, libdeflate {version()}, file of {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
