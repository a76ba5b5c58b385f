// Host program for tests/test_sam_host.py: csrc/sam_body.hpp compiled for the
// host (SAMX_HOST_ONLY) and run on one thread under -fsanitize=address,undefined.
// The kernels make a row's 64-bit masks by wave ballots and give each set bit to
// its lane; here a loop over the 64 bytes makes the masks and a loop over the set
// bits stands for the lanes. Everything else is sam_body.hpp's own text.
// The text lives in a heap block of exactly its length and the CIGAR words in a
// block of exactly their count, so a read or write past them is an error, not a
// silent success.
//
//   sam_host_main IN OUT
//
// IN:  the SAM text, byte for byte.
// OUT: "H n_header_lines n_records n_words", per record
//      "line_no line seq_off qual_off seq_len qual_len pos cigar n_cigar flag mapq mate_same_contig defect",
//      then "P word...". The lowest line with a syntax error ends the program
//      with status 3 after printing "E line_no code" to OUT.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "../../gatk-haplotypecaller-cpp17_amd/csrc/sam_body.hpp"

using namespace hcsam;

// Bit l: byte at + l lies before `end` and is not `what` (whitespace / a digit).
static uint64_t row_mask(const uint8_t* t, int64_t at, int64_t end, bool (*what)(uint8_t))
{
    uint64_t m = 0;
    for (int l = 0; l < 64 && at + l < end; ++l)
        if (!what(t[at + l])) m |= uint64_t(1) << l;
    return m;
}

// wave_cigar of sam_kernels.hip, the lanes one after the other.
static bool host_cigar(const uint8_t* t, int64_t cb, int64_t ce, uint32_t* words, int32_t& n, uint64_t& read_len)
{
    n = 0;
    read_len = 0;
    if (ce - cb == 1 && t[cb] == '*') return true;
    bool bad = sam_digit(t[ce - 1]);
    for (int64_t off = cb; off < ce; off += 64) {
        const uint64_t ops = row_mask(t, off, ce, sam_digit);
        for (uint64_t m = ops; m; m &= m - 1) {
            const int lane = sam_ctz(m);
            uint32_t word = 0;
            uint64_t len = 0;
            if (sam_element(t, cb, off + lane, word, len)) {
                read_len += len;
                if (words) words[n + __builtin_popcountll(ops & ((uint64_t(1) << lane) - 1))] = word;
            } else {
                bad = true;
            }
        }
        n += __builtin_popcountll(ops);
    }
    return !bad;
}

// sam_parse_kernel's work on one line.
static int32_t sam_line(const uint8_t* t, int64_t begin, int64_t end, hc_sam_record& o)
{
    if (end - begin > 0x7fffffffLL) return kErrLong;
    const int64_t len = end - begin;
    int32_t tok[2 * kFields];
    SamTokens tk(tok);
    for (int64_t off = 0; off < len && !tk.done(); off += 64) tk.row(row_mask(t, begin + off, end, sam_space), int32_t(off));
    tk.finish(int32_t(len));
    if (tk.n_end == 0) return kSkip;
    if (tk.n_end < kFields) return kErrFields;
    uint64_t val[5];
    uint32_t num_ok = 0;
    for (int j = 0; j < 5; ++j)
        if (sam_numeric(t, begin, tok, j, val[j])) num_ok |= 1u << j;
    int32_t n_cigar = 0;
    uint64_t read_len = 0;
    const bool cigar_ok = host_cigar(t, begin + tok[5], begin + tok[kFields + 5], nullptr, n_cigar, read_len);
    return sam_record(t, begin, tok, num_ok, val, cigar_ok, n_cigar, read_len, o);
}

// sam_emit_kernel's work on one line.
static void sam_words(const uint8_t* t, int64_t begin, int64_t end, int32_t cigar_off, uint32_t* words)
{
    const int64_t cb = begin + cigar_off;
    int64_t ce = end;
    for (int64_t off = cb; off < end; off += 64) {
        const uint64_t stop = ~row_mask(t, off, end, sam_space);
        if (stop) {
            ce = off + sam_ctz(stop);
            break;
        }
    }
    int32_t n = 0;
    uint64_t read_len = 0;
    (void)host_cigar(t, cb, ce, words, n, read_len);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    const std::string whole((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const int64_t len = int64_t(whole.size());
    std::unique_ptr<uint8_t[]> text(new uint8_t[size_t(len)]);   // no terminator, no slack
    for (int64_t i = 0; i < len; ++i) text[size_t(i)] = uint8_t(whole[size_t(i)]);
    std::ofstream out(argv[2]);

    // a line starts at byte 0 and after every newline that is not the last byte
    std::vector<int64_t> starts;
    for (int64_t i = 0; i < len; ++i)
        if (i == 0 || text[size_t(i - 1)] == '\n') starts.push_back(i);
    const int64_t n_lines = int64_t(starts.size());
    int64_t header = 0;
    while (header < n_lines && text[size_t(starts[size_t(header)])] == '@') ++header;

    std::vector<hc_sam_record> recs;
    std::vector<int64_t> rec_line;
    int64_t n_words = 0;
    for (int64_t k = header; k < n_lines; ++k) {
        hc_sam_record o;
        const int32_t e = sam_line(text.get(), starts[size_t(k)], sam_line_end(text.get(), len, starts.data(), k, n_lines), o);
        if (e == kSkip) continue;
        if (e != kErrNone) {
            out << "E " << k + 1 << ' ' << e << '\n';
            return 3;
        }
        recs.push_back(o);
        rec_line.push_back(k);
        n_words += o.n_cigar;
    }
    std::unique_ptr<uint32_t[]> pool(new uint32_t[size_t(n_words)]);
    int64_t word = 0;
    for (size_t r = 0; r < recs.size(); ++r) {
        hc_sam_record& o = recs[r];
        const int64_t k = rec_line[r];
        if (o.n_cigar)
            sam_words(text.get(), o.line, sam_line_end(text.get(), len, starts.data(), k, n_lines), o.cigar, pool.get() + word);
        o.cigar = int32_t(word);
        word += o.n_cigar;
    }
    out << "H " << header << ' ' << recs.size() << ' ' << n_words << '\n';
    for (size_t r = 0; r < recs.size(); ++r) {
        const hc_sam_record& o = recs[r];
        out << rec_line[r] + 1 << ' ' << o.line << ' ' << o.seq_off << ' ' << o.qual_off << ' ' << o.seq_len << ' ' << o.qual_len
            << ' ' << o.pos << ' ' << o.cigar << ' ' << o.n_cigar << ' ' << o.flag << ' ' << o.mapq << ' '
            << int(o.mate_same_contig) << ' ' << int(o.defect) << '\n';
    }
    out << 'P';
    for (int64_t w = 0; w < n_words; ++w) out << ' ' << pool[size_t(w)];
    out << '\n';
    return 0;
}
