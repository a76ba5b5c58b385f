// SAM parser kernels (include/hc_sam.h), gfx950. All integer, plain vector stores.
//
//   sam_lines_kernel<false>  one wave per 1024 bytes of text: every lane loads 16
//                            bytes, the wave lays them out in LDS and walks them
//                            in 16 rows of 64; a ballot over "byte is '\n'" gives
//                            the row's newline mask, shifted by one with the bit
//                            carried from the row before it is the mask of line
//                            starts. Counts the starts of the chunk.
//   sam_scan_*_kernel        exclusive scan of the counts: a sum per tile of 4096,
//                            the scan of the tile sums in one workgroup, the scan
//                            inside every tile on top of its base.
//   sam_lines_kernel<true>   the same walk; the lane of a start stores its offset
//                            at the scanned base plus the popcount of the lower
//                            lanes, and lowers header_end when its byte is not '@'.
//   sam_parse_kernel         one wave per line from header_end on, 64 bytes of the
//                            line per row: a ballot over "not whitespace" gives
//                            the masks of token starts and ends (sam_body.hpp),
//                            the five numbers are read by five lanes, the CIGAR
//                            by the wave (a ballot over "not a digit" is the mask
//                            of its operators, one lane per element). The record
//                            goes to a per-line slot, the line's record count
//                            (0 / 1) and CIGAR words are counted.
//   sam_scan_*_kernel        twice: records and words in front of every line.
//   sam_emit_kernel          one wave per line with a record: the record to its
//                            place, the CIGAR words into the pool, one lane per element.
//
// Every output position comes from a scan, none from the order of arrival, so
// records and pool are the same bytes on every run; the two atomicMin words
// (header_end, err) are minima and do not depend on the order either.
#include "sam_kernels.hpp"

namespace hcsam {

static_assert(sizeof(hc_sam_record) == 48, "hc_sam_record layout");

template <bool kWrite>
__global__ __launch_bounds__(64 * kWavesPerBlock) void sam_lines_kernel(SamArgs a)
{
    __shared__ uint4 rows[kWavesPerBlock][64];
    const int lane = int(threadIdx.x) & 63, wv = int(threadIdx.x) >> 6;
    const int64_t c = int64_t(blockIdx.x) * kWavesPerBlock + wv;
    const bool live = c < a.n_chunks;   // wave-uniform
    const int64_t base = c * kChunkBytes;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (live) v = reinterpret_cast<const uint4*>(a.text + base)[lane];
    rows[wv][lane] = v;
    __syncthreads();
    if (!live) return;
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(rows[wv]);
    // a line starts at the chunk's first byte when the byte before it is a newline
    unsigned long long carry = (base == 0 || a.text[base - 1] == '\n') ? 1ull : 0ull;
    int64_t at = kWrite ? a.chunk_first[c] : 0;
    int32_t count = 0;
    for (int r = 0; r < kChunkBytes / 64; ++r) {
        const int64_t i = base + r * 64 + lane;
        const uint8_t b = bytes[r * 64 + lane];
        const bool in = i < a.len;
        const unsigned long long valid = __ballot(in);
        const unsigned long long nl = __ballot(in && b == '\n');
        const unsigned long long starts = ((nl << 1) | carry) & valid;
        carry = nl >> 63;
        if (kWrite) {
            if ((starts >> lane) & 1ull) {
                const int64_t k = at + __popcll(starts & ((1ull << lane) - 1ull));
                a.line_start[k] = i;
                // nearly every line qualifies: only one that lowers the word goes to the atomic unit
                if (b != '@' && k < __atomic_load_n(a.header_end, __ATOMIC_RELAXED)) atomicMin(a.header_end, int32_t(k));
            }
            at += __popcll(starts);
        } else {
            count += __popcll(starts);
        }
    }
    if (!kWrite && lane == 0) a.chunk_lines[c] = count;
}

// The block's exclusive prefix of `v` in thread order and the block's total:
// wave scans by shuffles, the 16 wave totals through LDS.
__device__ inline int64_t block_exclusive(int64_t v, int64_t* wave_sums, int64_t& block_total)
{
    const int lane = int(threadIdx.x) & 63, wv = int(threadIdx.x) >> 6;
    int64_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t x = __shfl_up(inc, d, 64);
        if (lane >= d) inc += x;
    }
    if (lane == 63) wave_sums[wv] = inc;
    __syncthreads();
    int64_t before = 0, total = 0;
    for (int k = 0; k < kScanBlock / 64; ++k) {
        const int64_t s = wave_sums[k];
        if (k < wv) before += s;
        total += s;
    }
    __syncthreads();   // wave_sums is free for the next round
    block_total = total;
    return before + inc - v;
}

// Tile b = kScanTile elements, kScanPer consecutive ones per thread.
__global__ __launch_bounds__(kScanBlock) void sam_scan_sums_kernel(const int32_t* in, int64_t n, int64_t* sums)
{
    __shared__ int64_t wave_sums[kScanBlock / 64];
    const int64_t at = int64_t(blockIdx.x) * kScanTile + int64_t(threadIdx.x) * kScanPer;
    int64_t v = 0;
    for (int j = 0; j < kScanPer; ++j)
        if (at + j < n) v += in[at + j];
    int64_t total = 0;
    (void)block_exclusive(v, wave_sums, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// One workgroup: the exclusive scan of the tile sums, kScanBlock per round with a carry.
__global__ __launch_bounds__(kScanBlock) void sam_scan_top_kernel(const int64_t* sums, int64_t n_tiles, int64_t* first)
{
    __shared__ int64_t wave_sums[kScanBlock / 64];
    int64_t carry = 0;
    for (int64_t r = 0; r < n_tiles; r += kScanBlock) {
        const int64_t i = r + threadIdx.x;
        const int64_t v = i < n_tiles ? sums[i] : 0;
        int64_t total = 0;
        const int64_t before = block_exclusive(v, wave_sums, total);
        if (i < n_tiles) first[i] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) first[n_tiles] = carry;
}

__global__ __launch_bounds__(kScanBlock) void sam_scan_write_kernel(const int32_t* in, int64_t n, const int64_t* first,
                                                                    int64_t n_tiles, int64_t* out)
{
    __shared__ int64_t wave_sums[kScanBlock / 64];
    const int64_t at = int64_t(blockIdx.x) * kScanTile + int64_t(threadIdx.x) * kScanPer;
    int32_t x[kScanPer];
    int64_t v = 0;
    for (int j = 0; j < kScanPer; ++j) {
        x[j] = at + j < n ? in[at + j] : 0;
        v += x[j];
    }
    int64_t total = 0;
    int64_t run = block_exclusive(v, wave_sums, total);
    if (int64_t(blockIdx.x) < n_tiles) run += first[blockIdx.x];
    for (int j = 0; j < kScanPer; ++j) {
        if (at + j < n) out[at + j] = run;
        run += x[j];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = first[n_tiles];
}

// The CIGAR token [cb, ce) by the whole wave, 64 bytes per row: a ballot over
// "not a digit" is the mask of the operators, each operator's lane reads its
// element (sam_element) and, with `words`, stores it at the count of the rows
// before plus the popcount of the lower lanes. "*" is no element. False for
// anything that is not a CIGAR. n and read_len are the same in every lane.
__device__ inline bool wave_cigar(const uint8_t* t, int64_t cb, int64_t ce, uint32_t* words, int lane, int32_t& n,
                                  uint64_t& read_len)
{
    n = 0;
    read_len = 0;
    if (ce - cb == 1 && t[cb] == '*') return true;
    bool bad = sam_digit(t[ce - 1]);   // digits without an operator
    long long mine = 0;
    for (int64_t off = cb; off < ce; off += 64) {
        const int64_t i = off + lane;
        const bool op_here = i < ce && !sam_digit(t[i]);
        const unsigned long long ops = __ballot(op_here);
        if (op_here) {
            uint32_t word = 0;
            uint64_t len = 0;
            if (sam_element(t, cb, i, word, len)) {
                mine += static_cast<long long>(len);
                if (words) words[n + __popcll(ops & ((1ull << lane) - 1ull))] = word;
            } else {
                bad = true;
            }
        }
        n += __popcll(ops);
    }
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    read_len = static_cast<uint64_t>(mine);
    return __ballot(bad) == 0ull;
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void sam_parse_kernel(SamArgs a)
{
    __shared__ int32_t toks[kWavesPerBlock][2 * kFields];
    const int lane = int(threadIdx.x) & 63, wv = int(threadIdx.x) >> 6;
    const int64_t k = int64_t(blockIdx.x) * kWavesPerBlock + wv;
    if (k >= a.n_lines) return;   // wave-uniform, as is everything below that is not indexed by `lane`
    int32_t has = 0, words = 0;
    if (k >= *a.header_end) {
        const int64_t begin = a.line_start[k];
        const int64_t end = sam_line_end(a.text, a.len, a.line_start, k, a.n_lines);
        hc_sam_record o;
        int32_t e = kErrLong;
        if (end - begin <= 0x7fffffffLL) {
            const int64_t len = end - begin;
            SamTokens tk(toks[wv]);
            for (int64_t off = 0; off < len && !tk.done(); off += 64) {
                const int64_t i = off + lane;
                tk.row(__ballot(i < len && !sam_space(a.text[begin + i])), int32_t(off));
            }
            tk.finish(int32_t(len));
            if (tk.n_end == 0) {
                e = kSkip;
            } else if (tk.n_end < kFields) {
                e = kErrFields;
            } else {
                // the five numbers by five lanes, the CIGAR by the wave
                uint64_t v = 0;
                const bool ok = lane < 5 && sam_numeric(a.text, begin, tk.tok, lane, v);
                const uint32_t num_ok = uint32_t(__ballot(ok));
                uint64_t val[5];
                for (int j = 0; j < 5; ++j) val[j] = static_cast<uint64_t>(__shfl(static_cast<long long>(v), j, 64));
                int32_t n_cigar = 0;
                uint64_t read_len = 0;
                const bool cigar_ok =
                    wave_cigar(a.text, begin + tk.tok[5], begin + tk.tok[kFields + 5], nullptr, lane, n_cigar, read_len);
                e = sam_record(a.text, begin, tk.tok, num_ok, val, cigar_ok, n_cigar, read_len, o);
            }
        }
        if (e == kErrNone) {
            has = 1;
            words = o.n_cigar;
            if (lane == 0) a.tmp[k] = o;
        } else if (e != kSkip && lane == 0) {
            atomicMin(a.err, static_cast<unsigned long long>(k) * 16ull + static_cast<unsigned long long>(e));
        }
    }
    if (lane == 0) {
        a.has_record[k] = has;
        a.n_words[k] = words;
    }
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void sam_emit_kernel(SamArgs a)
{
    const int lane = int(threadIdx.x) & 63;
    const int64_t k = int64_t(blockIdx.x) * kWavesPerBlock + (int(threadIdx.x) >> 6);
    if (k >= a.n_lines || !a.has_record[k]) return;   // wave-uniform
    hc_sam_record o = a.tmp[k];
    const int64_t word = a.word_first[k];
    if (o.n_cigar) {
        const int64_t end = sam_line_end(a.text, a.len, a.line_start, k, a.n_lines);
        const int64_t cb = o.line + o.cigar;
        int64_t ce = end;   // the token ends at the first byte that is whitespace or past the line
        for (int64_t off = cb; off < end; off += 64) {
            const int64_t i = off + lane;
            const unsigned long long stop = ~__ballot(i < end && !sam_space(a.text[i]));
            if (stop) {
                ce = off + sam_ctz(stop);
                break;
            }
        }
        int32_t n = 0;
        uint64_t read_len = 0;
        (void)wave_cigar(a.text, cb, ce, a.pool + word, lane, n, read_len);
    }
    if (lane == 0) {
        o.cigar = int32_t(word);
        const int64_t r = a.rec_first[k];
        a.records[r] = o;
        a.line_no[r] = int32_t(k) + 1;
    }
}

static unsigned blocks_of(int64_t n, int per) { return unsigned((n + per - 1) / per); }

hipError_t launch_line_count(const SamArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(sam_lines_kernel<false>, dim3(blocks_of(a.n_chunks, kWavesPerBlock)), dim3(64 * kWavesPerBlock), 0,
                       st, a);
    return hipGetLastError();
}

hipError_t launch_line_write(const SamArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(sam_lines_kernel<true>, dim3(blocks_of(a.n_chunks, kWavesPerBlock)), dim3(64 * kWavesPerBlock), 0,
                       st, a);
    return hipGetLastError();
}

hipError_t launch_parse(const SamArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(sam_parse_kernel, dim3(blocks_of(a.n_lines, kWavesPerBlock)), dim3(64 * kWavesPerBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_emit(const SamArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(sam_emit_kernel, dim3(blocks_of(a.n_lines, kWavesPerBlock)), dim3(64 * kWavesPerBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_scan(const int32_t* in, int64_t n, int64_t* out, int64_t* work, hipStream_t st)
{
    const int64_t n_tiles = scan_tiles(n);
    int64_t* sums = work;
    int64_t* first = work + n_tiles;
    if (n_tiles) hipLaunchKernelGGL(sam_scan_sums_kernel, dim3(unsigned(n_tiles)), dim3(kScanBlock), 0, st, in, n, sums);
    hipLaunchKernelGGL(sam_scan_top_kernel, dim3(1), dim3(kScanBlock), 0, st, sums, n_tiles, first);
    hipLaunchKernelGGL(sam_scan_write_kernel, dim3(unsigned(n_tiles ? n_tiles : 1)), dim3(kScanBlock), 0, st, in, n, first,
                       n_tiles, out);
    return hipGetLastError();
}

}  // namespace hcsam
