// Host program for tests/test_bgzf_host.py: csrc/bgzf_body.hpp compiled for the
// host (BGZF_HOST_ONLY) and run on one thread under
// -fsanitize=address,undefined. bgzf_inflate_kernel gives a member to a wave of
// 64 lanes; here every per-lane piece runs 64 times in turn, and everything
// else is bgzf_body.hpp's own text: the header walk, the bit reader, the
// tables, the decode, the copies and the CRC32 by slices. The file, each
// member's DEFLATE stream and each member's output live in heap blocks of
// exactly their sizes, so a read or a write past them is an error, not a
// silent success.
//
//   bgzf_host_main IN.bgzf OUT.bin
//
// OUT.bin: the inflated bytes of the members in front of the first error.
// stdout:  one line "M index coff out_off isize" per such member, then
//          "E member code coff" for the first error (hcbgzf::BgzfError) or "OK".
//
//   bgzf_host_main --batch DIR N
//
// The files DIR/0.bgzf ... DIR/<N-1>.bgzf in one run: DIR/<k>.bin as OUT.bin
// above, and on stdout the last line alone for every file, in order.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>

#include "../../gatk-haplotypecaller-cpp17_amd/csrc/bgzf_body.hpp"

using namespace hcbgzf;

// One file. With `rows`, the member lines go to stdout; the last line ("E ..." or "OK") always does.
static int run(const char* in_path, const char* out_path, bool rows)
{
    std::ifstream in(in_path, std::ios::binary);
    if (!in) return 2;
    const std::string whole((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const int64_t len = int64_t(whole.size());
    std::unique_ptr<uint8_t[]> file(new uint8_t[size_t(len)]);
    std::memcpy(file.get(), whole.data(), size_t(len));
    std::ofstream out(out_path, std::ios::binary);
    std::unique_ptr<BgzfWork> work(new BgzfWork);
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; ++i) table[i] = bgzf_crc_entry(i);

    int64_t out_off = 0;
    int32_t index = 0;
    for (int64_t off = 0; off < len; ++index) {
        BgzfMember m{};
        int32_t err = bgzf_member_header(file.get(), len, off, m);
        if (!err) {
            m.out_off = out_off;
            const int32_t shift = int32_t(out_off & 15);
            std::unique_ptr<uint8_t[]> cdata(new uint8_t[size_t(m.cdata_len)]);
            std::memcpy(cdata.get(), file.get() + m.cdata, size_t(m.cdata_len));
            std::unique_ptr<uint8_t[]> bytes(new uint8_t[size_t(shift + m.isize)]);
            err = bgzf_inflate_member(*work, cdata.get(), m.cdata_len, bytes.get(), shift, m.isize);
            if (!err) {
                uint32_t crc = 0;
                for (int lane = 0; lane < 64; ++lane) crc ^= bgzf_crc_share(table, bytes.get() + shift, m.isize, lane);
                if ((crc ^ 0xFFFFFFFFu) != m.crc) err = kErrCrc;
            }
            if (!err) {
                out.write(reinterpret_cast<const char*>(bytes.get() + shift), m.isize);
                if (rows) std::printf("M %d %lld %lld %d\n", index, (long long)m.coff, (long long)m.out_off, m.isize);
            }
        }
        if (err) {
            std::printf("E %d %d %lld\n", index, err, (long long)off);
            return 0;
        }
        out_off += m.isize;
        off = m.cdata + m.cdata_len + 8;
    }
    std::printf("OK\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && std::strcmp(argv[1], "--batch") == 0) {
        const int count = std::atoi(argv[3]);
        for (int k = 0; k < count; ++k) {
            const std::string stem = std::string(argv[2]) + "/" + std::to_string(k);
            const int rc = run((stem + ".bgzf").c_str(), (stem + ".bin").c_str(), false);
            if (rc) return rc;
        }
        return 0;
    }
    if (argc != 3) return 2;
    return run(argv[1], argv[2], true);
}
