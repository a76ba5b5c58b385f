// The BGZF inflater's core (include/hc_bam.h), written once for the device and
// the host: a member's header, the bit reader, the canonical Huffman tables,
// the symbol decode, the copy rules of stored blocks and LZ77 matches, the
// copy-out and the CRC32 of a member by per-lane slices. bam_kernels.hip runs
// it with one wave per member; with BGZF_HOST_ONLY (no HIP header)
// tests/cpp/bgzf_host_main.cpp runs the same text on one thread under the host
// sanitizers, the compressed bytes and the output in heap blocks of exactly
// their sizes.
//
// How a wave is used. The decoder's state (bit buffer, positions, the current
// symbol) is the same in every lane: all 64 lanes read the same bytes and the
// same table entries and so agree on every branch. What differs per lane is
// written as BGZF_LANES(lane) { ... }: on the device the body runs once with
// the thread's own lane, on the host 64 times in turn. BGZF_SYNC() separates a
// phase that writes the workspace from one that reads what other lanes wrote
// (__syncthreads() of a one-wave block; nothing on the host). What the decoder
// loads (compressed words, table entries) goes through BGZF_UNIFORM, so that
// its state lives in scalar registers on the device. A literal is
// stored by lane 0. A match of `length` bytes at distance `dist` is copied by
// all lanes at once: byte k comes from pos - dist + k % dist, which lies before
// pos for every k, so no lane reads what another lane writes in the same copy
// (distance < length included). Stored blocks, the clearing and filling of the
// fast tables, the copy-out and the CRC32 run lane-parallel too; the counting
// sort of the code lengths (at most 320 steps per block) is lane 0's.
//
// Bounds. `in` is read at [0, in_len) only and `out` written at
// [shift, shift + isize) only. Every loop ends with the input or the output:
// a symbol consumes at least one bit, a block at least three, the slow decode
// at most 15 bits, and the symbol loop also carries an explicit budget of
// 8 * in_len + 8 rounds. An error ends the member at once with its code.
#pragma once
#ifdef BGZF_HOST_ONLY
#define BGZF_FN
#define BGZF_HD
#define BGZF_LANES(lane) for (int lane = 0; lane < 64; ++lane)
#define BGZF_SYNC() ((void)0)
#define BGZF_UNIFORM(x) (x)
#else
#include <hip/hip_runtime.h>
#define BGZF_FN __device__
#define BGZF_HD __host__ __device__
#define BGZF_LANES(lane) for (int lane = int(threadIdx.x) & 63, once_ = 1; once_; once_ = 0)
#define BGZF_SYNC() __syncthreads()
// A value every lane holds alike, said so to the compiler: what is computed from it stays in scalar
// registers and branches on it are scalar branches. Only where all lanes are active and agree.
#define BGZF_UNIFORM(x) __builtin_amdgcn_readfirstlane(int(x))
#endif

#include <cstdint>
#include <cstring>

namespace hcbgzf {

// A member's error word; 0 is none. The first three are found by the host's walk.
enum BgzfError : int32_t {
    kOk = 0,
    kErrHeader = 1,     // magic, CM, the FEXTRA flag, the BC subfield, a block shorter than its own fields
    kErrBsize = 2,      // BSIZE past the end of the file
    kErrIsize = 3,      // ISIZE above 65536
    kErrStream = 4,     // a malformed DEFLATE stream
    kErrEarly = 5,      // the stream ends before its last block does
    kErrCount = 6,      // the stream produces another byte count than ISIZE
    kErrDistance = 7,   // a back-reference before the member's first byte
    kErrCrc = 8,
};

constexpr int32_t kMaxIsize = 65536;
constexpr int kLitBits = 10, kDistBits = 8;   // of the fast tables
constexpr int kMaxLit = 288, kMaxDist = 32;
constexpr int kOutPad = 16;                   // `out` begins at shift = (its place in the file's inflated bytes) & 15

struct BgzfMember {
    int64_t coff;        // of the member in the file
    int64_t cdata;       // of its DEFLATE stream in the file
    int64_t out_off;     // of its bytes in the inflated stream
    int32_t cdata_len;
    int32_t isize;
    uint32_t crc;
    int32_t reserved;
};

BGZF_HD inline uint32_t bgzf_le16(const uint8_t* p) { return uint32_t(p[0]) | uint32_t(p[1]) << 8; }
BGZF_HD inline uint32_t bgzf_le32(const uint8_t* p)
{
    return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}

// The member that begins at file[off] (off < len). Fills m but out_off.
BGZF_HD inline int32_t bgzf_member_header(const uint8_t* file, int64_t len, int64_t off, BgzfMember& m)
{
    const uint8_t* p = file + off;
    const int64_t left = len - off;
    if (left < 12 || p[0] != 31u || p[1] != 139u || p[2] != 8u || !(p[3] & 4u)) return kErrHeader;
    const int64_t xlen = bgzf_le16(p + 10);
    if (left < 12 + xlen) return kErrHeader;
    int64_t bsize = -1;
    for (int64_t x = 0; x + 4 <= xlen;) {   // at most xlen / 4 subfields
        const int64_t slen = bgzf_le16(p + 12 + x + 2);
        if (p[12 + x] == 66u && p[12 + x + 1] == 67u) {
            if (slen != 2 || x + 6 > xlen) return kErrHeader;
            bsize = int64_t(bgzf_le16(p + 12 + x + 4)) + 1;
            break;
        }
        x += 4 + slen;
    }
    if (bsize < 0 || bsize < 12 + xlen + 8) return kErrHeader;
    if (bsize > left) return kErrBsize;
    m.coff = off;
    m.cdata = off + 12 + xlen;
    m.cdata_len = int32_t(bsize - 12 - xlen - 8);
    m.crc = bgzf_le32(p + bsize - 8);
    const uint32_t isize = bgzf_le32(p + bsize - 4);
    m.isize = isize > uint32_t(kMaxIsize) ? kMaxIsize + 1 : int32_t(isize);
    m.reserved = 0;
    return isize > uint32_t(kMaxIsize) ? kErrIsize : kOk;
}

// ---- CRC32 (the reflected polynomial 0xEDB88320) -------------------------------------

constexpr uint32_t kCrcPoly = 0xEDB88320u;

BGZF_HD inline uint32_t bgzf_crc_entry(uint32_t i)
{
    for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ kCrcPoly : i >> 1;
    return i;
}

// a * b mod P; bit 31 is x^0.
BGZF_HD inline uint32_t bgzf_crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int k = 0; k < 32; ++k) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}

// x^(8 n) mod P, 0 <= n <= 65536.
BGZF_HD inline uint32_t bgzf_crc_xpow8(uint32_t n)
{
    uint32_t r = 0x80000000u, base = 0x00800000u;   // 1 and x^8
    for (int k = 0; k < 17; ++k) {
        if ((n >> k) & 1u) r = bgzf_crc_mul(r, base);
        base = bgzf_crc_mul(base, base);
    }
    return r;
}

// The shift register run over p[0, n) from `state`, without the final inversion.
BGZF_HD inline uint32_t bgzf_crc_bytes(const uint32_t* table, const uint8_t* p, int32_t n, uint32_t state)
{
    for (int32_t i = 0; i < n; ++i) state = table[(state ^ p[i]) & 255u] ^ (state >> 8);
    return state;
}

// Lane `lane`'s share of the CRC32 of p[0, n): the register after its slice
// (lane 0 begins at ~0, the others at 0) times x^(8 * the bytes behind the
// slice). The XOR of the 64 shares, inverted, is the CRC32.
BGZF_HD inline uint32_t bgzf_crc_share(const uint32_t* table, const uint8_t* p, int32_t n, int lane)
{
    const int32_t slice = (n + 63) / 64;
    const int32_t b = lane * slice < n ? lane * slice : n;
    const int32_t e = b + slice < n ? b + slice : n;
    const uint32_t s = bgzf_crc_bytes(table, p + b, e - b, lane == 0 ? 0xFFFFFFFFu : 0u);
    return s ? bgzf_crc_mul(s, bgzf_crc_xpow8(uint32_t(n - e))) : 0u;
}

// ---- the inflater ----------------------------------------------------------------------

// The wave's workspace (LDS on the device) beside the output block.
struct BgzfWork {
    uint16_t lit_fast[1 << kLitBits];    // (symbol << 4) | length of a code of up to kLitBits bits, 0: the slow way
    uint16_t dist_fast[1 << kDistBits];
    uint16_t lit_sym[kMaxLit], dist_sym[kMaxDist], cl_sym[19];   // the symbols in canonical order
    uint16_t lit_count[16], dist_count[16], cl_count[16];        // codes per length
    uint16_t first[16], offs[16];        // of the table being built: the first code and its place per length
    uint8_t lens[kMaxLit + kMaxDist];
    int32_t status;                      // lane 0's verdict on a table
};

struct BgzfBits {
    const uint8_t* p;
    int32_t len, at;   // `at`: the next byte to load
    uint64_t hold;
    int32_t n;         // valid bits in hold; the bits above them are 0
    bool early;        // more bits were asked for than the stream has

    BGZF_FN void refill()
    {
        if (n > 32) return;
        if (at + 4 <= len) {
            uint32_t w;
            std::memcpy(&w, p + at, 4);
            hold |= uint64_t(uint32_t(BGZF_UNIFORM(w))) << n;
            n += 32;
            at += 4;
            return;
        }
        for (; at < len; ++at, n += 8) hold |= uint64_t(uint32_t(BGZF_UNIFORM(p[at]))) << n;   // at most three bytes
    }
    BGZF_FN void drop(int k)
    {
        if (k > n) {
            early = true;
            k = n;
        }
        hold >>= k;
        n -= k;
    }
    BGZF_FN uint32_t take(int k)   // k <= 16
    {
        const uint32_t v = uint32_t(hold) & ((1u << k) - 1u);
        drop(k);
        return v;
    }
};

BGZF_FN inline uint32_t bgzf_rev(uint32_t code, int len)
{
    uint32_t r = 0;
    for (int k = 0; k < len; ++k) r |= ((code >> k) & 1u) << (len - 1 - k);
    return r;
}

// The decode tables of w.lens[at, at + n): count[] and sym[] (the canonical
// order, for codes longer than the fast table's index) and, with fast_bits > 0,
// the fast table. What zlib refuses is refused: an over-subscribed set, and an
// incomplete one unless its only codes are one bit long.
BGZF_FN inline int32_t bgzf_build(BgzfWork& w, int at, int n, uint16_t* count, uint16_t* sym, uint16_t* fast, int fast_bits)
{
    BGZF_LANES(lane)
    {
        if (lane == 0) {
            for (int l = 0; l < 16; ++l) count[l] = 0;
            for (int s = 0; s < n; ++s) ++count[w.lens[at + s]];
            int32_t left = 1, max = 0;
            for (int l = 1; l < 16; ++l) {
                left = (left << 1) - int32_t(count[l]);
                if (left < 0) break;
                if (count[l]) max = l;
            }
            w.status = left < 0 || (left > 0 && max > 1) ? kErrStream : kOk;
            uint32_t code = 0, off = 0;
            for (int l = 1; l < 16; ++l) {
                w.first[l] = uint16_t(code);
                w.offs[l] = uint16_t(off);
                code = (code + count[l]) << 1;
                off += count[l];
            }
            if (w.status == kOk) {
                uint16_t next[16];
                for (int l = 1; l < 16; ++l) next[l] = w.offs[l];
                for (int s = 0; s < n; ++s)
                    if (w.lens[at + s]) sym[next[w.lens[at + s]]++] = uint16_t(s);
            }
        }
        if (fast_bits)
            for (int k = lane; k < (1 << fast_bits); k += 64) fast[k] = 0;
    }
    BGZF_SYNC();
    const int32_t status = BGZF_UNIFORM(w.status);
    if (status != kOk) return status;
    if (fast_bits) {
        const int coded = n - BGZF_UNIFORM(count[0]);
        BGZF_LANES(lane)
        {
            for (int i = lane; i < coded; i += 64) {
                const uint32_t s = sym[i];
                const int l = w.lens[at + s];
                if (l > fast_bits) continue;
                const uint32_t code = uint32_t(w.first[l]) + uint32_t(i - int(w.offs[l]));
                for (uint32_t k = bgzf_rev(code, l); k < (1u << fast_bits); k += 1u << l) fast[k] = uint16_t(s << 4 | uint32_t(l));
            }
        }
        BGZF_SYNC();
    }
    return kOk;
}

// One symbol, or -1 for a bit pattern that is no code; b.early when the stream ends inside it.
BGZF_FN inline int32_t bgzf_decode(BgzfBits& b, const uint16_t* fast, int fast_bits, const uint16_t* count, const uint16_t* sym)
{
    if (fast_bits) {
        const uint32_t e = uint32_t(BGZF_UNIFORM(fast[uint32_t(b.hold) & ((1u << fast_bits) - 1u)]));
        if (e) {
            b.drop(int(e & 15u));
            return int32_t(e >> 4);
        }
    }
    int32_t code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
        code |= int32_t(b.hold >> (l - 1)) & 1;
        const int32_t c = BGZF_UNIFORM(count[l]);
        if (code - c < first) {
            b.drop(l);
            return BGZF_UNIFORM(sym[index + (code - first)]);
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    if (b.n < 15) b.early = true;
    return -1;
}

// One member. `in` = its DEFLATE stream, in_len bytes. The bytes go to
// out[shift, shift + isize). Returns kOk when the stream is well formed and
// gave isize bytes exactly.
BGZF_FN inline int32_t bgzf_inflate_member(BgzfWork& w, const uint8_t* in, int32_t in_len, uint8_t* out, int32_t shift,
                                           int32_t isize)
{
    BgzfBits b{in, in_len, 0, 0, 0, false};
    int32_t pos = 0;
    int64_t budget = int64_t(in_len) * 8 + 8;   // rounds of the symbol loop, over all blocks
    for (int32_t blocks = in_len * 8 / 3 + 1; blocks > 0; --blocks) {
        b.refill();
        const uint32_t last = b.take(1), type = b.take(2);
        if (b.early) return kErrEarly;
        if (type == 3u) return kErrStream;
        if (type == 0u) {
            b.drop(b.n & 7);
            b.refill();
            const uint32_t n = b.take(16), inv = b.take(16);
            if (b.early) return kErrEarly;
            if ((n ^ inv) != 0xFFFFu) return kErrStream;
            const int32_t from = b.at - b.n / 8;   // hold has whole bytes only
            if (from + int32_t(n) > in_len) return kErrEarly;
            if (pos + int32_t(n) > isize) return kErrCount;
            BGZF_LANES(lane)
            {
                for (int32_t k = lane; k < int32_t(n); k += 64) out[shift + pos + k] = in[from + k];
            }
            pos += int32_t(n);
            b.at = from + int32_t(n);
            b.hold = 0;
            b.n = 0;
        } else {
            if (type == 1u) {
                BGZF_LANES(lane)
                {
                    for (int s = lane; s < kMaxLit + kMaxDist; s += 64)
                        w.lens[s] = uint8_t(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < kMaxLit ? 8 : 5);
                }
                BGZF_SYNC();
                (void)bgzf_build(w, 0, kMaxLit, w.lit_count, w.lit_sym, w.lit_fast, kLitBits);
                (void)bgzf_build(w, kMaxLit, kMaxDist, w.dist_count, w.dist_sym, w.dist_fast, kDistBits);
            } else {
                const int32_t nlen = int32_t(b.take(5)) + 257, ndist = int32_t(b.take(5)) + 1, ncode = int32_t(b.take(4)) + 4;
                if (b.early) return kErrEarly;
                if (nlen > 286 || ndist > 30) return kErrStream;
                uint32_t cl[19];
                for (int k = 0; k < 19; ++k) {
                    if (k < ncode && (k & 7) == 0) b.refill();
                    cl[k] = k < ncode ? b.take(3) : 0u;
                }
                if (b.early) return kErrEarly;
                BGZF_SYNC();   // the last block's tables are no longer read
                BGZF_LANES(lane)
                {
                    if (lane == 0) {
                        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
                        for (int k = 0; k < 19; ++k) w.lens[order[k]] = uint8_t(cl[k]);
                    }
                }
                BGZF_SYNC();
                if (BGZF_UNIFORM(bgzf_build(w, 0, 19, w.cl_count, w.cl_sym, nullptr, 0)) != kOk) return kErrStream;
                // the code lengths, decoded by every lane alike into registers' worth of state and stored by lane 0
                BGZF_SYNC();
                int32_t have = 0, prev = 0;
                while (have < nlen + ndist) {   // every round adds at least one length
                    b.refill();
                    const int32_t s = bgzf_decode(b, nullptr, 0, w.cl_count, w.cl_sym);
                    if (b.early) return kErrEarly;
                    if (s < 0) return kErrStream;
                    int32_t rep = 1, val = s;
                    if (s == 16) {
                        if (have == 0) return kErrStream;
                        val = prev;
                        rep = 3 + int32_t(b.take(2));
                    } else if (s == 17) {
                        val = 0;
                        rep = 3 + int32_t(b.take(3));
                    } else if (s == 18) {
                        val = 0;
                        rep = 11 + int32_t(b.take(7));
                    }
                    if (b.early) return kErrEarly;
                    if (have + rep > nlen + ndist) return kErrStream;
                    BGZF_LANES(lane)
                    {
                        // after the build below, lens[0, 288) are the literal / length codes' and lens[288, 320) the distances'
                        for (int32_t k = lane; k < rep; k += 64) {
                            const int32_t i = have + k;
                            w.lens[i < nlen ? i : kMaxLit + (i - nlen)] = uint8_t(val);
                        }
                    }
                    have += rep;
                    prev = val;
                }
                BGZF_LANES(lane)
                {
                    for (int s = nlen + lane; s < kMaxLit; s += 64) w.lens[s] = 0;
                    for (int s = ndist + lane; s < kMaxDist; s += 64) w.lens[kMaxLit + s] = 0;
                }
                BGZF_SYNC();
                if (BGZF_UNIFORM(w.lens[256]) == 0) return kErrStream;   // no end-of-block code
                if (BGZF_UNIFORM(bgzf_build(w, 0, kMaxLit, w.lit_count, w.lit_sym, w.lit_fast, kLitBits)) != kOk) return kErrStream;
                if (BGZF_UNIFORM(bgzf_build(w, kMaxLit, kMaxDist, w.dist_count, w.dist_sym, w.dist_fast, kDistBits)) != kOk) return kErrStream;
            }
            for (;;) {
                if (--budget < 0) return kErrStream;
                b.refill();
                const int32_t s = bgzf_decode(b, w.lit_fast, kLitBits, w.lit_count, w.lit_sym);
                if (b.early) return kErrEarly;
                if (s < 0) return kErrStream;
                if (s < 256) {
                    if (pos >= isize) return kErrCount;
                    BGZF_LANES(lane)
                    {
                        if (lane == 0) out[shift + pos] = uint8_t(s);
                    }
                    ++pos;
                    continue;
                }
                if (s == 256) break;
                const int32_t c = s - 257;
                if (c > 28) return kErrStream;
                int32_t length;
                if (c < 8) {
                    length = 3 + c;
                } else if (c == 28) {
                    length = 258;
                } else {
                    const int e = (c >> 2) - 1;
                    length = 3 + ((4 + (c & 3)) << e) + int32_t(b.take(e));
                }
                b.refill();
                const int32_t d = bgzf_decode(b, w.dist_fast, kDistBits, w.dist_count, w.dist_sym);
                if (b.early) return kErrEarly;
                if (d < 0 || d > 29) return kErrStream;
                int32_t dist;
                if (d < 4) {
                    dist = 1 + d;
                } else {
                    const int e = (d >> 1) - 1;
                    dist = 1 + ((2 + (d & 1)) << e) + int32_t(b.take(e));
                }
                if (b.early) return kErrEarly;
                if (dist > pos) return kErrDistance;
                if (pos + length > isize) return kErrCount;
                BGZF_SYNC();   // lane 0's literals are in place
                BGZF_LANES(lane)
                {
                    const int32_t from = shift + pos - dist;
                    for (int32_t k = lane; k < length; k += 64) out[shift + pos + k] = out[from + (dist < length ? k % dist : k)];
                }
                BGZF_SYNC();
                pos += length;
            }
        }
        if (last) return pos == isize ? kOk : kErrCount;
    }
    return kErrEarly;
}

}  // namespace hcbgzf
