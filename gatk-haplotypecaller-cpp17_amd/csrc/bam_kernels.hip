// BAM front kernels (include/hc_bam.h), gfx950. All integer, plain vector stores.
//
//   bgzf_inflate_kernel   one wave (a block of 64) per BGZF member, the text of
//                         bgzf_body.hpp: the decoder's state is the same in all
//                         lanes, lane 0 stores literals, all lanes copy matches,
//                         stored blocks and table entries. The member's output
//                         (at most 64 KiB) and the decode tables live in LDS, so
//                         a back-reference is an LDS read; two blocks share a CU.
//                         The output sits in LDS at the member's place modulo 16
//                         in the inflated stream, so the copy-out moves aligned
//                         16-byte pieces from LDS to global memory, the ragged
//                         ends byte by byte. A member with an error writes its
//                         error word and nothing else.
//   bgzf_crc_kernel       one wave per member over the inflated bytes: every lane
//                         runs the byte-wise table CRC over its 1/64 slice and
//                         multiplies by x^(8 * bytes behind it) mod P; the XOR of
//                         the shares is the CRC32 (bgzf_crc_share).
//   bam_decode_kernel     one wave per alignment record, framed by the host:
//                         CIGAR words to the pool, SEQ nibbles to ASCII and QUAL
//                         + 33 to the bases buffer with lane-contiguous reads and
//                         stores, the CIGAR's read length and the quality range by
//                         wave reductions, the record by lane 0.
//   bam_contig_of_kernel  one lane per record: ref_id through the reference map.
#include "bam_kernels.hpp"

#include "sam_body.hpp"

namespace hcbam {

using namespace hcbgzf;

__global__ __launch_bounds__(64) void bgzf_inflate_kernel(InflateArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t out[kMaxIsize + kOutPad];
    __shared__ BgzfWork work;
    const int32_t m = int32_t(blockIdx.x);
    if (m >= a.n_members) return;
    const BgzfMember mem = a.members[m];
    const int lane = int(threadIdx.x) & 63;
    const int32_t shift = BGZF_UNIFORM(mem.out_off & 15), isize = BGZF_UNIFORM(mem.isize);
    const int32_t err = bgzf_inflate_member(work, a.file + mem.cdata, BGZF_UNIFORM(mem.cdata_len), out, shift, isize);
    __syncthreads();
    if (lane == 0) a.err[m] = err;
    if (err != kOk) return;
    uint8_t* base = a.out + (mem.out_off - shift);   // 16-byte aligned, as out[] is
    const int32_t end = shift + isize;
    for (int32_t p = lane * 16; p < end; p += 64 * 16) {
        if (p >= shift && p + 16 <= end) {
            *reinterpret_cast<uint4*>(base + p) = *reinterpret_cast<const uint4*>(out + p);
        } else {
            for (int32_t i = p < shift ? shift : p; i < p + 16 && i < end; ++i) base[i] = out[i];
        }
    }
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void bgzf_crc_kernel(InflateArgs a)
{
    __shared__ uint32_t table[256];
    for (uint32_t i = threadIdx.x; i < 256u; i += 64 * kWavesPerBlock) table[i] = bgzf_crc_entry(i);
    __syncthreads();
    const int lane = int(threadIdx.x) & 63;
    const int32_t m = int32_t(blockIdx.x) * kWavesPerBlock + (int(threadIdx.x) >> 6);
    if (m >= a.n_members || a.err[m] != kOk) return;   // wave-uniform
    const BgzfMember mem = a.members[m];
    uint32_t share = bgzf_crc_share(table, a.out + mem.out_off, mem.isize, lane);
    for (int d = 32; d >= 1; d >>= 1) share ^= uint32_t(__shfl_xor(int(share), d, 64));
    if (lane == 0 && (share ^ 0xFFFFFFFFu) != mem.crc) a.err[m] = kErrCrc;
}

__device__ inline uint32_t le32(const uint8_t* p) { return bgzf_le32(p); }

__global__ __launch_bounds__(64 * kWavesPerBlock) void bam_decode_kernel(DecodeArgs a)
{
    const int lane = int(threadIdx.x) & 63;
    const int64_t k = int64_t(blockIdx.x) * kWavesPerBlock + (int(threadIdx.x) >> 6);
    if (k >= a.n_records) return;   // wave-uniform, as is everything below that is not indexed by `lane`
    const uint8_t* r = a.stream + a.rec_off[k];
    const int32_t ref_id = int32_t(le32(r + kRefId)), next_ref_id = int32_t(le32(r + kNextRefId));
    const int32_t l_name = r[kLName], n_cigar = int32_t(bgzf_le16(r + kNCigar)), l_seq = int32_t(le32(r + kLSeq));
    const int64_t cf = a.cigar_first[k], bf = a.bases_first[k];

    const uint8_t* cigar = r + kName + l_name;
    unsigned long long read_len = 0;
    bool bad_op = false;
    for (int32_t i = lane; i < n_cigar; i += 64) {
        const uint32_t w = le32(cigar + 4 * int64_t(i));
        a.pool[cf + i] = w;
        const uint32_t op = w & 15u;
        bad_op |= op > 8u;
        if (op <= 8u && ((hcsam::kReadOps >> op) & 1u)) read_len += w >> 4;
    }
    for (int d = 32; d >= 1; d >>= 1) read_len += __shfl_xor(read_len, d, 64);
    if (__any(bad_op) && lane == 0) atomicMin(a.err, static_cast<unsigned long long>(k) * 16ull + kErrCigarOp);

    const uint8_t* seq = cigar + 4 * int64_t(n_cigar);
    const uint8_t* qual = seq + (int64_t(l_seq) + 1) / 2;
    const bool no_qual = l_seq > 0 && qual[0] == 0xFFu;
    bool high = false;
    for (int32_t j = lane; j < l_seq; j += 64) {
        const uint32_t b = seq[j >> 1];
        a.bases[bf + j] = uint8_t("=ACMGRSVTWYHKDBN"[(j & 1) ? (b & 15u) : (b >> 4)]);
        const uint32_t q = qual[j];
        a.bases[bf + l_seq + j] = uint8_t(q + 33u);
        high |= q > 93u;
    }
    const bool any_high = __any(high) != 0;
    if (lane != 0) return;
    hc_sam_record o{};
    o.line = bf;
    o.seq_off = 0;
    o.qual_off = uint32_t(l_seq);
    o.seq_len = l_seq;
    o.qual_len = no_qual ? 0 : l_seq;
    o.pos = uint32_t(le32(r + kPos)) + 1u;
    o.cigar = int32_t(cf);
    o.n_cigar = n_cigar;
    o.flag = uint16_t(bgzf_le16(r + kFlag));
    o.mapq = r[kMapq];
    o.mate_same_contig = (next_ref_id == ref_id && ref_id >= 0) ? 1 : 0;
    o.defect = o.pos == 0                                    ? HC_SAM_DEFECT_POS_ZERO
               : n_cigar == 0                                ? HC_SAM_DEFECT_NO_CIGAR
               : read_len != (unsigned long long)(l_seq)     ? HC_SAM_DEFECT_CIGAR_LENGTH
               : o.qual_len != o.seq_len                     ? HC_SAM_DEFECT_QUAL_LENGTH
               : l_seq > HC_PHMM_MAX_READ_LEN                ? HC_SAM_DEFECT_TOO_LONG
               : (!no_qual && any_high)                      ? HC_SAM_DEFECT_QUAL_RANGE
                                                             : HC_SAM_DEFECT_NONE;
    a.records[k] = o;
    a.line_no[k] = int32_t(k) + 1;
    a.ref_id[k] = ref_id;
}

__global__ __launch_bounds__(256) void bam_contig_of_kernel(const int32_t* ref_id, const int32_t* ref_contig, int32_t n_records,
                                                            int32_t* contig_of)
{
    const int64_t k = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (k >= n_records) return;
    const int32_t r = ref_id[k];
    contig_of[k] = r < 0 ? -1 : ref_contig[r];
}

static unsigned blocks_of(int64_t n, int per) { return unsigned((n + per - 1) / per); }

hipError_t launch_inflate(const InflateArgs& a, hipStream_t st)
{
    if (a.n_members <= 0) return hipSuccess;
    hipLaunchKernelGGL(bgzf_inflate_kernel, dim3(unsigned(a.n_members)), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_crc(const InflateArgs& a, hipStream_t st)
{
    if (a.n_members <= 0) return hipSuccess;
    hipLaunchKernelGGL(bgzf_crc_kernel, dim3(blocks_of(a.n_members, kWavesPerBlock)), dim3(64 * kWavesPerBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_decode(const DecodeArgs& a, hipStream_t st)
{
    if (a.n_records <= 0) return hipSuccess;
    hipLaunchKernelGGL(bam_decode_kernel, dim3(blocks_of(a.n_records, kWavesPerBlock)), dim3(64 * kWavesPerBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_contig_of(const int32_t* ref_id, const int32_t* ref_contig, int32_t n_records, int32_t* contig_of,
                            hipStream_t st)
{
    if (n_records <= 0) return hipSuccess;
    hipLaunchKernelGGL(bam_contig_of_kernel, dim3(blocks_of(n_records, 256)), dim3(256), 0, st, ref_id, ref_contig, n_records,
                       contig_of);
    return hipGetLastError();
}

}  // namespace hcbam
