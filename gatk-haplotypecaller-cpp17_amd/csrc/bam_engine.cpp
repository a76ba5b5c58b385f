// Host engine + C ABI of the BAM front (include/hc_bam.h).
//
// One call, under the SAM parser's lock and on its stream:
//
//   members:   one walk over the compressed file (bgzf_member_header: the header
//              and the trailer of every member), the exclusive sum of ISIZE
//   upload:    the file through the parser's pinned staging block
//   inflate:   one wave per member (bam_kernels.hip), then the CRC32 per member;
//              one small readback: the members' error words
//   frame:     (BAM) the inflated stream back to the host, the header and the
//              block_size chain walked there, per record its offset and the
//              exclusive sums of n_cigar_op and 2 * l_seq sent up
//   decode:    one wave per record: records, ordinals, refIDs, the CIGAR pool and
//              the bases buffer; one readback of all five
//
// hc_bam_genome_call is a front of the genome caller (genome_engine.hpp): the
// records stay on the device with the bases buffer in the text's place, and
// contig_of comes from refID through a map of the header's references into the
// caller's table. hc_bam_genome_call_intervals with an index (include/hc_intervals.h)
// reads the header's members, chooses chunks on the host (bai.hpp), follows BSIZE
// through their members only, uploads those packed, and frames chunk by chunk.
// The workspace is the front's own: grow-only buffers of the
// shared host layer, released by hc_phmm_shutdown. HC_BAM_TRACE=1 prints the
// phases of hc_bgzf_inflate and hc_bam_parse on stderr.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hc_bam.h"
#include "bai.hpp"
#include "bam_kernels.hpp"
#include "genome_engine.hpp"
#include "sam_engine.hpp"
#include "stage_host.hpp"

using namespace hcbam;
using namespace hcbgzf;
using namespace stage_host;

struct hc_bgzf_result {
    std::vector<uint8_t> bytes;
    std::vector<int64_t> coff, ioff;
    std::vector<int32_t> isize;
};

namespace {

// What a BAM file gives beside the records.
struct BamExtras {
    std::vector<int32_t> ref_id;       // per record
    std::vector<std::string> names;    // the header's reference table
    std::vector<int64_t> lens;
    std::string text;                  // the header text
    std::vector<uint8_t> bases;
};

}  // namespace

struct hc_bam_result {
    hc_sam_result sam;
    BamExtras x;
};

namespace {

// No stream and no lock of its own: the kernels run on the parser's, under the parser's lock.
Buf g_infl, g_meta, g_frame, g_out, g_map, g_hmeta{nullptr, 0, true}, g_hinfl{nullptr, 0, true}, g_hframe{nullptr, 0, true},
    g_hout{nullptr, 0, true}, g_hmap{nullptr, 0, true};
Stage g_st({&g_infl, &g_meta, &g_frame, &g_out, &g_map, &g_hmeta, &g_hinfl, &g_hframe, &g_hout, &g_hmap}, false);

const char* container_text(int32_t code)
{
    switch (code) {
        case kErrHeader: return "not a BGZF member (magic, the FEXTRA flag or the BC subfield)";
        case kErrBsize: return "BSIZE reaches past the end of the file";
        case kErrIsize: return "ISIZE above 65536";
        case kErrStream: return "a malformed DEFLATE stream";
        case kErrEarly: return "the DEFLATE stream ends early";
        case kErrCount: return "the DEFLATE stream does not produce ISIZE bytes";
        case kErrDistance: return "a back-reference before the member's first byte";
        case kErrCrc: return "CRC32 mismatch";
        default: return "unknown device error";
    }
}

int container_error(int64_t member, int64_t off, int32_t code)
{
    return fail(HC_PHMM_EINVAL, "member " + std::to_string(member) + " at offset " + std::to_string(off) + ": " + container_text(code));
}

struct Inflated {
    std::vector<BgzfMember> members;
    int64_t total = 0;              // inflated bytes
    const uint8_t* dev = nullptr;   // they, on the device
};

// inf.members (offsets into the `len` bytes of the pieces put one behind the other, out_off set, inf.total their
// sum) inflated on the device and their CRC32 checked. true_off: per member its offset in the file where the
// pieces are a packed choice of it, else null. mark: whether the phases enter the trace.
int inflate_list(const std::vector<hcsam::Piece>& pieces, int64_t len, Inflated& inf, const std::vector<int64_t>* true_off, Trace& tr,
                 bool mark = true)
{
    hipStream_t st = hcsam::parser_stage().stream;
    const size_t n = inf.members.size();
    if (!n) return HC_PHMM_OK;
    const uint8_t* dev_file = nullptr;
    int rc = hcsam::upload_pieces(pieces.data(), pieces.size(), len, size_t(len), dev_file);
    if (rc) return rc;
    if (mark) tr.mark("upload");
    rc = reserve(g_infl, up(size_t(inf.total)) + 256, "inflated bytes on the device");
    if (rc) return rc;
    Carver mc;
    const size_t o_mem = mc.take(sizeof(BgzfMember) * n);
    const size_t o_err = mc.take(sizeof(int32_t) * n);
    rc = reserve(g_meta, mc.off, "BGZF member table on the device");
    if (rc) return rc;
    rc = reserve(g_hmeta, mc.off, "BGZF member table staging");
    if (rc) return rc;
    std::memcpy(g_hmeta.p + o_mem, inf.members.data(), sizeof(BgzfMember) * n);
    HIP_TRY(st, hipMemcpyAsync(g_meta.p + o_mem, g_hmeta.p + o_mem, sizeof(BgzfMember) * n, hipMemcpyHostToDevice, st));
    InflateArgs a{};
    a.file = dev_file;
    a.members = reinterpret_cast<const BgzfMember*>(g_meta.p + o_mem);
    a.n_members = int32_t(n);
    a.out = reinterpret_cast<uint8_t*>(g_infl.p);
    a.err = reinterpret_cast<int32_t*>(g_meta.p + o_err);
    HIP_TRY(st, launch_inflate(a, st));
    if (tr.on && mark) {
        HIP_TRY(st, hipStreamSynchronize(st));
        tr.mark("inflate");
    }
    HIP_TRY(st, launch_crc(a, st));
    HIP_TRY(st, hipMemcpyAsync(g_hmeta.p + o_err, a.err, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(st, hipStreamSynchronize(st));
    if (mark) tr.mark("crc");
    const int32_t* err = reinterpret_cast<const int32_t*>(g_hmeta.p + o_err);
    for (size_t m = 0; m < n; ++m)
        if (err[m] != kOk) return container_error(int64_t(m), true_off ? (*true_off)[m] : inf.members[m].coff, err[m]);
    inf.dev = a.out;
    return HC_PHMM_OK;
}

// The members of `file` inflated on the device and their CRC32 checked. With the parser's lock held and its stage ready.
int inflate_on_device(const uint8_t* file, int64_t len, Inflated& inf, Trace& tr)
{
    int32_t pending = kOk;   // what the walk stopped at: it loses to an error of a member in front of it
    int64_t pending_off = 0;
    for (int64_t off = 0; off < len;) {
        BgzfMember m{};
        pending = bgzf_member_header(file, len, off, m);
        pending_off = off;
        if (pending != kOk) break;
        if (inf.members.size() >= 0x7fffffffu) return fail(HC_PHMM_EINVAL, "more than 2147483647 BGZF members");
        m.out_off = inf.total;
        inf.total += m.isize;
        inf.members.push_back(m);
        off = m.cdata + m.cdata_len + 8;
    }
    const size_t n = inf.members.size();
    if (int rc = inflate_list({hcsam::Piece{file, len}}, len, inf, nullptr, tr)) return rc;
    if (pending != kOk) return container_error(int64_t(n), pending_off, pending);
    tr.value("members", double(n));
    tr.value("file_bytes", double(len));
    tr.value("inflated_bytes", double(inf.total));
    return HC_PHMM_OK;
}

// The inflated bytes in the pinned block g_hinfl.
int inflated_to_host(const Inflated& inf)
{
    hipStream_t st = hcsam::parser_stage().stream;
    int rc = reserve(g_hinfl, size_t(std::max<int64_t>(inf.total, 1)), "inflated bytes readback");
    if (rc) return rc;
    if (inf.total) {
        HIP_TRY(st, hipMemcpyAsync(g_hinfl.p, inf.dev, size_t(inf.total), hipMemcpyDeviceToHost, st));
        HIP_TRY(st, hipStreamSynchronize(st));
    }
    return HC_PHMM_OK;
}

int32_t rd32(const uint8_t* p) { return int32_t(bgzf_le32(p)); }

// The BAM header at the front of s[0, total): 0 and `at` behind it, 1 when the
// stream ends inside it (`need`: the bytes it has to have at least), 2 for any other error; `message` names both.
int header_of(const uint8_t* s, int64_t total, BamExtras& x, int64_t& at, std::string& message, int64_t& need)
{
    const std::string cut = "BAM header: cut short by the end of the stream";
    x.names.clear();
    x.lens.clear();
    if (total >= 4 && std::memcmp(s, "BAM\1", 4) != 0) {
        message = "BAM header: missing BAM\\1 magic";
        return 2;
    }
    if (total < 4) {
        message = "BAM header: missing BAM\\1 magic";
        need = 4;
        return total == 0 || std::memcmp(s, "BAM\1", size_t(total)) == 0 ? 1 : 2;
    }
    at = 4;
    if (at + 4 > total) {
        message = cut;
        need = at + 4;
        return 1;
    }
    const int64_t l_text = rd32(s + at);
    at += 4;
    if (l_text < 0) {
        message = "BAM header: a negative length";
        return 2;
    }
    if (at + l_text + 4 > total) {
        message = cut;
        need = at + l_text + 4;
        return 1;
    }
    x.text.assign(reinterpret_cast<const char*>(s + at), size_t(l_text));
    at += l_text;
    const int64_t n_ref = rd32(s + at);
    at += 4;
    if (n_ref < 0) {
        message = "BAM header: a negative length";
        return 2;
    }
    for (int64_t k = 0; k < n_ref; ++k) {
        if (at + 4 > total) {
            message = cut;
            need = at + 4;
            return 1;
        }
        const int64_t l_name = rd32(s + at);
        if (l_name < 1) {
            message = "BAM header: a reference name without its terminator";
            return 2;
        }
        if (at + 4 + l_name + 4 > total) {
            message = cut;
            need = at + 8 + l_name;
            return 1;
        }
        x.names.emplace_back(reinterpret_cast<const char*>(s + at + 4), strnlen(reinterpret_cast<const char*>(s + at + 4), size_t(l_name)));
        x.lens.push_back(rd32(s + at + 4 + l_name));
        at += 8 + l_name;
    }
    return 0;
}

// "record N: " of the record that begins at s[at].
using Where = std::function<std::string(size_t ordinal, int64_t at)>;

// The block_size chain of s[at, total), appended to the three lists. An error
// stops the walk: `message` names it, and the records in front of it are still
// decoded (an error of theirs comes first).
void records_of(const uint8_t* s, int64_t at, int64_t total, int64_t n_ref, std::vector<int64_t>& rec_off,
                std::vector<int64_t>& cigar_first, std::vector<int64_t>& bases_first, std::string& message, const Where& where_of)
{
    const std::string cut = "cut short by the end of the stream";
    while (at < total) {
        const auto where = [&] { return where_of(rec_off.size() + 1, at); };   // made for an error only
        const char* small = "block_size smaller than the record's own fields need";
        if (at + 4 > total) {
            message = where() + cut;
            return;
        }
        const int64_t bs = rd32(s + at);
        if (bs < 32) {
            message = where() + small;
            return;
        }
        if (at + 4 + bs > total) {
            message = where() + cut;
            return;
        }
        const uint8_t* r = s + at;
        const int64_t ref_id = rd32(r + kRefId), next_ref_id = rd32(r + kNextRefId), l_name = r[kLName];
        const int64_t n_cigar = bgzf_le16(r + kNCigar), l_seq = rd32(r + kLSeq);
        if (l_name == 0) {
            message = where() + "l_read_name is 0";
            return;
        }
        if (l_seq < 0 || 32 + l_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq > bs) {
            message = where() + small;
            return;
        }
        if (ref_id < -1 || ref_id >= n_ref || next_ref_id < -1 || next_ref_id >= n_ref) {
            message = where() + (ref_id < -1 || ref_id >= n_ref ? "refID" : "next_refID") + " outside -1 .. n_ref - 1";
            return;
        }
        if (rec_off.size() >= 0x7f000000u) {
            message = "more than 2130706432 records";
            return;
        }
        if (cigar_first.back() + n_cigar > 0x7fffffffLL) {
            message = "more than 2147483647 CIGAR elements";
            return;
        }
        rec_off.push_back(at);
        cigar_first.push_back(cigar_first.back() + n_cigar);
        bases_first.push_back(bases_first.back() + 2 * l_seq);
        at += 4 + bs;
    }
}


// The header and the block_size chain of the inflated stream s[0, total).
void frame(const uint8_t* s, int64_t total, BamExtras& x, std::vector<int64_t>& rec_off, std::vector<int64_t>& cigar_first,
           std::vector<int64_t>& bases_first, std::string& message)
{
    cigar_first.assign(1, 0);
    bases_first.assign(1, 0);
    int64_t at = 0, need = 0;
    if (header_of(s, total, x, at, message, need)) return;
    records_of(s, at, total, int64_t(x.names.size()), rec_off, cigar_first, bases_first, message,
               [](size_t n, int64_t) { return "record " + std::to_string(n) + ": "; });
}

int decode_resident(const Inflated& inf, const std::vector<int64_t>& rec_off, const std::vector<int64_t>& cigar_first,
                    const std::vector<int64_t>& bases_first, const std::string& message, hc_sam_result& sam, BamExtras& x,
                    hcsam::Resident& dev, const int32_t*& dev_ref_id, Trace& tr, const Where& where_of);

// hc_bam_parse with the records left on the device. With the parser's lock held and its stage ready.
int bam_resident(const uint8_t* file, int64_t len, hc_sam_result& sam, BamExtras& x, hcsam::Resident& dev,
                 const int32_t*& dev_ref_id, Trace& tr)
{
    Inflated inf;
    int rc = inflate_on_device(file, len, inf, tr);
    if (rc) return rc;
    rc = inflated_to_host(inf);
    if (rc) return rc;
    std::vector<int64_t> rec_off, cigar_first, bases_first;
    std::string message;
    frame(reinterpret_cast<const uint8_t*>(g_hinfl.p), inf.total, x, rec_off, cigar_first, bases_first, message);
    tr.mark("frame");
    return decode_resident(inf, rec_off, cigar_first, bases_first, message, sam, x, dev, dev_ref_id, tr,
                           [](size_t n, int64_t) { return "record " + std::to_string(n) + ": "; });
}

// The framed records of inf's stream decoded on the device and left there. `message` is the walk's error, if any.
int decode_resident(const Inflated& inf, const std::vector<int64_t>& rec_off, const std::vector<int64_t>& cigar_first,
                    const std::vector<int64_t>& bases_first, const std::string& message, hc_sam_result& sam, BamExtras& x,
                    hcsam::Resident& dev, const int32_t*& dev_ref_id, Trace& tr, const Where& where_of)
{
    hipStream_t st = hcsam::parser_stage().stream;
    int rc = HC_PHMM_OK;
    const size_t n = rec_off.size();
    const int64_t n_words = cigar_first.back(), n_bases = bases_first.back();

    Carver fc;
    const size_t f_off = fc.take(sizeof(int64_t) * n);
    const size_t f_cf = fc.take(sizeof(int64_t) * (n + 1));
    const size_t f_bf = fc.take(sizeof(int64_t) * (n + 1));
    rc = reserve(g_frame, fc.off, "BAM record offsets on the device");
    if (rc) return rc;
    rc = reserve(g_hframe, fc.off, "BAM record offsets staging");
    if (rc) return rc;
    Carver oc;
    const size_t o_err = oc.take(sizeof(unsigned long long));
    const size_t o_rec = oc.take(sizeof(hc_sam_record) * n);
    const size_t o_ln = oc.take(sizeof(int32_t) * n);
    const size_t o_ref = oc.take(sizeof(int32_t) * n);
    const size_t o_pool = oc.take(sizeof(uint32_t) * size_t(n_words));
    const size_t o_bases = oc.take(size_t(n_bases));
    rc = reserve(g_out, oc.off, "BAM records on the device");
    if (rc) return rc;
    rc = reserve(g_hout, oc.off, "BAM records readback");
    if (rc) return rc;
    if (n) std::memcpy(g_hframe.p + f_off, rec_off.data(), sizeof(int64_t) * n);
    std::memcpy(g_hframe.p + f_cf, cigar_first.data(), sizeof(int64_t) * (n + 1));
    std::memcpy(g_hframe.p + f_bf, bases_first.data(), sizeof(int64_t) * (n + 1));
    HIP_TRY(st, hipMemcpyAsync(g_frame.p, g_hframe.p, fc.off, hipMemcpyHostToDevice, st));
    DecodeArgs a{};
    a.stream = inf.dev;
    a.rec_off = reinterpret_cast<const int64_t*>(g_frame.p + f_off);
    a.cigar_first = reinterpret_cast<const int64_t*>(g_frame.p + f_cf);
    a.bases_first = reinterpret_cast<const int64_t*>(g_frame.p + f_bf);
    a.n_records = int32_t(n);
    a.records = reinterpret_cast<hc_sam_record*>(g_out.p + o_rec);
    a.line_no = reinterpret_cast<int32_t*>(g_out.p + o_ln);
    a.ref_id = reinterpret_cast<int32_t*>(g_out.p + o_ref);
    a.pool = reinterpret_cast<uint32_t*>(g_out.p + o_pool);
    a.bases = reinterpret_cast<uint8_t*>(g_out.p + o_bases);
    a.err = reinterpret_cast<unsigned long long*>(g_out.p + o_err);
    HIP_TRY(st, hipMemsetAsync(a.err, 0xFF, sizeof(unsigned long long), st));
    HIP_TRY(st, launch_decode(a, st));
    if (tr.on) {
        HIP_TRY(st, hipStreamSynchronize(st));
        tr.mark("decode");
    }
    HIP_TRY(st, hipMemcpyAsync(g_hout.p, g_out.p, oc.off, hipMemcpyDeviceToHost, st));
    HIP_TRY(st, hipStreamSynchronize(st));
    tr.mark("readback");
    unsigned long long err = 0;
    std::memcpy(&err, g_hout.p + o_err, sizeof(err));
    if (err != kNoError) {
        if ((err >> 4) >= n) return fail(HC_PHMM_EHIP, "BAM decode: error word out of its bound");
        return fail(HC_PHMM_EINVAL, where_of(size_t(err >> 4) + 1, rec_off[size_t(err >> 4)]) + "a CIGAR op above 8");
    }
    if (!message.empty()) return fail(HC_PHMM_EINVAL, message);
    const hc_sam_record* hr = reinterpret_cast<const hc_sam_record*>(g_hout.p + o_rec);
    const int32_t* hl = reinterpret_cast<const int32_t*>(g_hout.p + o_ln);
    const int32_t* hf = reinterpret_cast<const int32_t*>(g_hout.p + o_ref);
    const uint32_t* hp = reinterpret_cast<const uint32_t*>(g_hout.p + o_pool);
    const uint8_t* hb = reinterpret_cast<const uint8_t*>(g_hout.p + o_bases);
    sam.records.assign(hr, hr + n);
    sam.line_no.assign(hl, hl + n);
    sam.pool.assign(hp, hp + n_words);
    x.ref_id.assign(hf, hf + n);
    x.bases.assign(hb, hb + n_bases);
    tr.value("records", double(n));
    tr.value("bases_bytes", double(n_bases));
    dev.stream = st;
    dev.records = a.records;
    dev.line_no = a.line_no;
    dev.n_records = int32_t(n);
    dev.text = a.bases;
    dev.text_len = n_bases;
    dev_ref_id = a.ref_id;
    return HC_PHMM_OK;
}

int check_file(const uint8_t* file, int64_t len)
{
    return len < 0 || (len && !file) ? fail(HC_PHMM_EINVAL, "null file / negative length") : HC_PHMM_OK;
}

// hc_bam_genome_call's front.
struct BamFront : hcgenome::Front {
    const uint8_t* file;
    int64_t len;
    BamExtras x;
    hc_genome_result* res = nullptr;
    const int32_t* dev_ref_id = nullptr;
    BamFront(const uint8_t* f, int64_t n) : file(f), len(n) {}
    int check() const override { return check_file(file, len); }
    int open(hc_genome_result& r, const hcgenome::Table& t, Trace& tr, std::unique_lock<std::mutex>& lk,
             hcsam::Resident& dev) override
    {
        Stage& ps = hcsam::parser_stage();
        std::unique_lock<std::mutex> mine(ps.mu);
        if (int rc = ps.ensure_init()) return rc;
        if (tr.on) tr.line += " front=bam";
        res = &r;
        r.sam = new hc_sam_result();
        if (int rc = bam_resident(file, len, *r.sam, x, dev, dev_ref_id, tr)) return rc;
        r.bases.swap(x.bases);
        if (int rc = map_refs(t)) return rc;
        lk = std::move(mine);
        return HC_PHMM_OK;
    }
    // The header's references in the caller's table: ref_contig on the host (g_hmap) and on the device (g_map).
    int map_refs(const hcgenome::Table& t)
    {
        Stage& ps = hcsam::parser_stage();
        const size_t n_ref = std::max<size_t>(x.names.size(), 1);
        int rc = reserve(g_map, sizeof(int32_t) * n_ref, "BAM reference map on the device");
        if (rc) return rc;
        rc = reserve(g_hmap, sizeof(int32_t) * n_ref, "BAM reference map staging");
        if (rc) return rc;
        int32_t* map = reinterpret_cast<int32_t*>(g_hmap.p);
        const hcgenome::GenomeTable view = t.view();
        for (size_t k = 0; k < x.names.size(); ++k) {
            const std::string& s = x.names[k];
            uint32_t slot = 0;
            map[k] = s.empty() || s.size() > HC_GENOME_MAX_NAME_LEN
                         ? -1
                         : hcgenome::genome_lookup(view, reinterpret_cast<const uint8_t*>(s.data()), int64_t(s.size()), slot);
        }
        HIP_TRY(ps.stream, hipMemcpyAsync(g_map.p, g_hmap.p, sizeof(int32_t) * n_ref, hipMemcpyHostToDevice, ps.stream));
        HIP_TRY(ps.stream, hipStreamSynchronize(ps.stream));
        return HC_PHMM_OK;
    }
    hipError_t resolve(const hcgenome::GenomeArgs& a, hipStream_t st) override
    {
        return launch_contig_of(dev_ref_id, reinterpret_cast<const int32_t*>(g_map.p), a.n_records, a.contig_of, st);
    }
    const uint8_t* text() const override { return res->bases.data(); }
    std::string where(int64_t line_no) const override { return "record " + std::to_string(line_no) + ": "; }
    std::string rname(const hc_sam_record&, size_t k) const override
    {
        const int32_t r = x.ref_id[k];
        return r < 0 ? std::string("*") : x.names[size_t(r)].substr(0, 64);
    }
};

// hc_bam_genome_call_intervals' front with an index (include/hc_intervals.h): the header's members, then only
// the members that the chunks of the asked ranges lie in.
struct IndexedBamFront final : BamFront {
    const uint8_t* bai;
    int64_t bai_len;
    std::vector<BgzfMember> read;      // the members of the chunks, offsets into the packed copy
    std::vector<int64_t> true_off;     // per member of `read`: its offset in the file
    std::vector<int64_t> rec_at;       // per record: its offset in the inflated bytes of `read`
    IndexedBamFront(const uint8_t* f, int64_t n, const uint8_t* b, int64_t bn) : BamFront(f, n), bai(b), bai_len(bn) {}
    int check() const override
    {
        if (int rc = check_file(file, len)) return rc;
        return !bai || bai_len < 0 ? fail(HC_PHMM_EINVAL, "BAI: null index / negative length") : HC_PHMM_OK;
    }
    // The virtual offset of inflated offset `at` of the members read.
    uint64_t voffset(int64_t at) const
    {
        size_t lo = 0, hi = read.size();
        while (lo + 1 < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            if (read[mid].out_off <= at)
                lo = mid;
            else
                hi = mid;
        }
        return read.empty() ? 0 : uint64_t(true_off[lo]) << 16 | uint64_t(at - read[lo].out_off);
    }
    std::string where_at(size_t ordinal, int64_t at) const
    {
        return "record " + std::to_string(ordinal) + " (virtual offset " + std::to_string(voffset(at)) + "): ";
    }
    std::string where(int64_t line_no) const override
    {
        return line_no >= 1 && size_t(line_no) <= rec_at.size() ? where_at(size_t(line_no), rec_at[size_t(line_no) - 1])
                                                                 : BamFront::where(line_no);
    }
    // Members from offset 0 until the BAM header is whole: per round as many more as the
    // header is known to need, so the last one read is the one the header ends in.
    int read_header(Trace& tr, int64_t& header_bytes, int32_t& header_members)
    {
        Inflated inf;
        int64_t off = 0, need = 1;
        for (;;) {
            const size_t had = inf.members.size();
            while (off < len && inf.total < need) {
                BgzfMember m{};
                const int32_t code = bgzf_member_header(file, len, off, m);
                if (code != kOk) return container_error(int64_t(inf.members.size()), off, code);
                m.out_off = inf.total;
                inf.total += m.isize;
                inf.members.push_back(m);
                off = m.cdata + m.cdata_len + 8;
            }
            if (int rc = inflate_list({hcsam::Piece{file, off}}, off, inf, nullptr, tr, false)) return rc;   // under header=
            if (int rc = inflated_to_host(inf)) return rc;
            int64_t at = 0;
            std::string message;
            const int state = header_of(reinterpret_cast<const uint8_t*>(g_hinfl.p), inf.total, x, at, message, need);
            if (state == 0) {
                header_bytes = off;
                header_members = int32_t(inf.members.size());
                return HC_PHMM_OK;
            }
            if (state == 2 || (off >= len && inf.members.size() == had) || (off >= len && inf.total < need))
                return fail(HC_PHMM_EINVAL, message);
        }
    }
    int open(hc_genome_result& r, const hcgenome::Table& t, Trace& tr, std::unique_lock<std::mutex>& lk,
             hcsam::Resident& dev) override
    {
        Stage& ps = hcsam::parser_stage();
        std::unique_lock<std::mutex> mine(ps.mu);
        if (int rc = ps.ensure_init()) return rc;
        if (tr.on) tr.line += " front=bam";
        res = &r;
        r.sam = new hc_sam_result();
        int64_t header_bytes = 0;
        int32_t header_members = 0;
        if (int rc = read_header(tr, header_bytes, header_members)) return rc;
        if (int rc = map_refs(t)) return rc;
        tr.mark("header");

        // ---- the chunks of the runs of asked windows, chosen on the host
        hcbai::Index idx;
        const std::string bad = hcbai::bai_parse(bai, bai_len, int64_t(x.names.size()), len, idx);
        if (!bad.empty()) return fail(HC_PHMM_EINVAL, bad);
        const int32_t* map = reinterpret_cast<const int32_t*>(g_hmap.p);
        std::vector<int32_t> ref_of(r.names.size(), -1);   // a contig's refID: the first reference that maps to it
        for (size_t k = x.names.size(); k-- > 0;)
            if (map[k] >= 0) ref_of[size_t(map[k])] = int32_t(k);
        std::vector<hcbai::Chunk> chunks;
        const hcgenome::Merged& m = r.merged;
        for (size_t c = 0; c < r.names.size(); ++c) {
            // the merged intervals ascend, so the windows they ask for ascend: a run ends where the next interval's first window is not its neighbour
            for (int32_t k = m.first[c]; k < m.first[c + 1];) {
                const int64_t w0 = m.begin[size_t(k)] / r.region;
                int64_t w1 = (m.end[size_t(k)] - 1) / r.region;
                for (++k; k < m.first[c + 1] && m.begin[size_t(k)] / r.region <= w1 + 1; ++k) w1 = (m.end[size_t(k)] - 1) / r.region;
                const int64_t beg = w0 == 0 ? 0 : w0 * r.region - r.padding;
                const int64_t end = std::min((w1 + 1) * r.region + r.padding, r.ref_len[c]);
                if (end > hcbai::kMaxPos)   // the unindexed call would read those records: no silent difference
                    return fail(HC_PHMM_EINVAL, "BAI: contig " + r.names[c] + " is asked past position 536870912, which a .bai does not reach");
                if (ref_of[c] >= 0 && beg < end) hcbai::bai_query(idx, ref_of[c], beg, end, chunks);
            }
        }
        hcbai::bai_merge(chunks);

        // ---- BSIZE from each chunk's first member to the member its end lands in; every offset checked against the file
        std::vector<hcsam::Piece> pieces;   // per chunk its members' bytes, as they lie in the file
        int64_t packed = 0;
        std::vector<std::pair<int64_t, int64_t>> span;   // per chunk: [from, to) in the inflated bytes of `read`
        Inflated inf;
        for (const hcbai::Chunk& ch : chunks) {
            const int64_t c_end = int64_t(ch.end >> 16), u_beg = int64_t(ch.beg & 0xffff), u_end = int64_t(ch.end & 0xffff);
            const int64_t first_out = inf.total;
            const int64_t from = int64_t(ch.beg >> 16);
            int64_t off = from, last_out = -1, last_isize = 0, first_isize = -1;
            while (off < len && (off < c_end || (off == c_end && u_end > 0))) {   // parse checked beg, end < len
                BgzfMember mem{};
                const int32_t code = bgzf_member_header(file, len, off, mem);
                if (code != kOk) return container_error(int64_t(inf.members.size()), off, code);
                if (inf.members.size() >= 0x7fffffffu) return fail(HC_PHMM_EINVAL, "more than 2147483647 BGZF members");
                const int64_t next = mem.cdata + mem.cdata_len + 8;
                true_off.push_back(off);
                mem.out_off = inf.total;
                mem.cdata = packed + (mem.cdata - from);
                mem.coff = packed + (off - from);
                if (first_isize < 0) first_isize = mem.isize;
                last_out = mem.out_off;
                last_isize = mem.isize;
                inf.total += mem.isize;
                inf.members.push_back(mem);
                off = next;
            }
            const std::string at = "BAI: chunk at virtual offset " + std::to_string(ch.beg) + ": ";
            if (off < c_end || (off > c_end && !(u_end > 0 && last_out >= 0 && true_off.back() == c_end)))
                return fail(HC_PHMM_EINVAL, at + "its end is at no member of the file");
            if (off > from) {   // bgzf_member_header kept every member inside the file
                pieces.push_back(hcsam::Piece{file + from, off - from});
                packed += off - from;
            }
            if (first_isize < 0) {   // an empty chunk inside one member's front
                if (ch.beg != ch.end) return fail(HC_PHMM_EINVAL, at + "it holds no member");
                continue;
            }
            if (u_beg > first_isize || u_end > last_isize) return fail(HC_PHMM_EINVAL, at + "an offset past its member's bytes");
            const int64_t to = u_end > 0 ? last_out + u_end : inf.total;
            if (first_out + u_beg > to) return fail(HC_PHMM_EINVAL, at + "it ends in front of its begin");
            span.emplace_back(first_out + u_beg, to);
        }
        tr.mark("index");
        read = inf.members;
        if (int rc = inflate_list(pieces, packed, inf, &true_off, tr)) return rc;
        if (int rc = inflated_to_host(inf)) return rc;

        // ---- frame chunk by chunk, decode, and the rest as the plain front
        std::vector<int64_t> cigar_first(1, 0), bases_first(1, 0);
        std::string message;
        const Where where_of = [this](size_t n, int64_t at) { return where_at(n, at); };
        for (const auto& sp : span) {
            records_of(reinterpret_cast<const uint8_t*>(g_hinfl.p), sp.first, sp.second, int64_t(x.names.size()), rec_at, cigar_first,
                       bases_first, message, where_of);
            if (!message.empty()) break;
        }
        tr.mark("frame");
        if (int rc = decode_resident(inf, rec_at, cigar_first, bases_first, message, *r.sam, x, dev, dev_ref_id, tr, where_of))
            return rc;
        r.bases.swap(x.bases);
        r.idx_chunks = int32_t(span.size());
        r.idx_members = header_members + int32_t(read.size());
        r.idx_bytes_up = header_bytes + packed;
        r.idx_records = int64_t(rec_at.size());
        tr.count("chunks", r.idx_chunks);
        tr.count("members", r.idx_members);
        tr.count("bytes_up", r.idx_bytes_up);
        lk = std::move(mine);
        return HC_PHMM_OK;
    }
};

}  // namespace

extern "C" int hc_bgzf_inflate(const uint8_t* file, int64_t file_len, hc_bgzf_result** out)
{
    Stage& ps = hcsam::parser_stage();
    std::lock_guard<std::mutex> lk(ps.mu);
    return call_frame(out, &ps.stream, [&](hc_bgzf_result& res) -> int {
        if (int rc = check_file(file, file_len)) return rc;
        if (int rc = ps.ensure_init()) return rc;
        Trace tr("HC_BAM_TRACE", "[hc_bam]");
        Inflated inf;
        if (int rc = inflate_on_device(file, file_len, inf, tr)) return rc;
        if (int rc = inflated_to_host(inf)) return rc;
        tr.mark("readback");
        const uint8_t* h = reinterpret_cast<const uint8_t*>(g_hinfl.p);
        res.bytes.assign(h, h + inf.total);
        for (const BgzfMember& m : inf.members) {
            res.coff.push_back(m.coff);
            res.ioff.push_back(m.out_off);
            res.isize.push_back(m.isize);
        }
        return HC_PHMM_OK;
    });
}

extern "C" int hc_bgzf_result_bytes(const hc_bgzf_result* res, const uint8_t** bytes, int64_t* length)
{
    if (!res) return fail(HC_PHMM_EINVAL, "null result");
    if (bytes) *bytes = res->bytes.data();
    if (length) *length = int64_t(res->bytes.size());
    return HC_PHMM_OK;
}

extern "C" int hc_bgzf_result_members(const hc_bgzf_result* res, const int64_t** compressed_offset,
                                      const int64_t** inflated_offset, const int32_t** isize, int32_t* n_members)
{
    if (!res) return fail(HC_PHMM_EINVAL, "null result");
    if (compressed_offset) *compressed_offset = res->coff.data();
    if (inflated_offset) *inflated_offset = res->ioff.data();
    if (isize) *isize = res->isize.data();
    if (n_members) *n_members = int32_t(res->isize.size());
    return HC_PHMM_OK;
}

extern "C" int hc_bgzf_result_free(hc_bgzf_result* res)
{
    delete res;
    return HC_PHMM_OK;
}

extern "C" int hc_bam_parse(const uint8_t* file, int64_t file_len, hc_bam_result** out)
{
    Stage& ps = hcsam::parser_stage();
    std::lock_guard<std::mutex> lk(ps.mu);
    return call_frame(out, &ps.stream, [&](hc_bam_result& res) -> int {
        if (int rc = check_file(file, file_len)) return rc;
        if (int rc = ps.ensure_init()) return rc;
        Trace tr("HC_BAM_TRACE", "[hc_bam]");
        hcsam::Resident dev;
        const int32_t* dev_ref_id = nullptr;
        return bam_resident(file, file_len, res.sam, res.x, dev, dev_ref_id, tr);
    });
}

extern "C" int hc_bam_result_records(const hc_bam_result* res, const hc_sam_record** records, const int32_t** line_no,
                                     int32_t* n_records, const uint32_t** cigar_pool, int32_t* n_words, const int32_t** ref_id)
{
    if (!res) return fail(HC_PHMM_EINVAL, "null result");
    if (ref_id) *ref_id = res->x.ref_id.data();
    return hc_sam_result_records(&res->sam, records, line_no, n_records, cigar_pool, n_words, nullptr);
}

extern "C" int hc_bam_result_header(const hc_bam_result* res, const char** text, int64_t* text_len, int32_t* n_ref)
{
    if (!res) return fail(HC_PHMM_EINVAL, "null result");
    if (text) *text = res->x.text.c_str();
    if (text_len) *text_len = int64_t(res->x.text.size());
    if (n_ref) *n_ref = int32_t(res->x.names.size());
    return HC_PHMM_OK;
}

extern "C" int hc_bam_result_reference(const hc_bam_result* res, int32_t ref, const char** name, int32_t* name_len,
                                       int64_t* length)
{
    if (!res) return fail(HC_PHMM_EINVAL, "null result");
    if (ref < 0 || size_t(ref) >= res->x.names.size()) return fail(HC_PHMM_EINVAL, "reference index out of range");
    if (name) *name = res->x.names[size_t(ref)].c_str();
    if (name_len) *name_len = int32_t(res->x.names[size_t(ref)].size());
    if (length) *length = res->x.lens[size_t(ref)];
    return HC_PHMM_OK;
}

extern "C" int hc_bam_result_bases(const hc_bam_result* res, const uint8_t** bases, int64_t* length)
{
    if (!res) return fail(HC_PHMM_EINVAL, "null result");
    if (bases) *bases = res->x.bases.data();
    if (length) *length = int64_t(res->x.bases.size());
    return HC_PHMM_OK;
}

extern "C" int hc_bam_result_free(hc_bam_result* res)
{
    delete res;
    return HC_PHMM_OK;
}

extern "C" int hc_bam_genome_call(const uint8_t* file, int64_t file_len, const hc_genome_contig* contigs, int32_t n_contigs,
                                  int32_t region_size, int32_t padding_size, uint64_t seed, int32_t pick_mode, uint32_t flags,
                                  hc_genome_result** out)
{
    BamFront front(file, file_len);
    return hcgenome::genome_call(front, contigs, n_contigs, region_size, padding_size, seed, pick_mode, flags, out);
}

// include/hc_intervals.h: the plain front plus the scope, or the indexed front.
extern "C" int hc_bam_genome_call_intervals(const uint8_t* file, int64_t file_len, const uint8_t* bai, int64_t bai_len,
                                            const hc_genome_contig* contigs, int32_t n_contigs, const hc_interval* intervals,
                                            int32_t n_intervals, int32_t region_size, int32_t padding_size, uint64_t seed,
                                            int32_t pick_mode, uint32_t flags, hc_genome_result** out)
{
    const hcgenome::Asking ask{intervals, n_intervals};
    if (!bai && bai_len == 0) {
        BamFront front(file, file_len);
        return hcgenome::genome_call(front, contigs, n_contigs, region_size, padding_size, seed, pick_mode, flags, out, &ask);
    }
    IndexedBamFront front(file, file_len, bai, bai_len);
    return hcgenome::genome_call(front, contigs, n_contigs, region_size, padding_size, seed, pick_mode, flags, out, &ask);
}

extern "C" int hc_bam_genome_result_index(const hc_genome_result* res, int32_t* n_chunks, int32_t* n_members, int64_t* bytes_up,
                                          int64_t* n_records)
{
    if (!res) return fail(HC_PHMM_EINVAL, "null result");
    if (n_chunks) *n_chunks = res->idx_chunks;
    if (n_members) *n_members = res->idx_members;
    if (bytes_up) *bytes_up = res->idx_bytes_up;
    if (n_records) *n_records = res->idx_records;
    return HC_PHMM_OK;
}

extern "C" int hc_bam_genome_result_bases(const hc_genome_result* res, const uint8_t** bases, int64_t* length)
{
    if (!res) return fail(HC_PHMM_EINVAL, "null result");
    if (bases) *bases = res->bases.empty() ? nullptr : res->bases.data();
    if (length) *length = int64_t(res->bases.size());
    return HC_PHMM_OK;
}
