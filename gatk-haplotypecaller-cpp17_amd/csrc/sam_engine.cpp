// Host engine + C ABI of the SAM parser (include/hc_sam.h).
//
// One call = every alignment line of a SAM text to a record:
//
//   the text goes up through one pinned staging block, piece after piece
//   line starts:   count per 1 KiB chunk, scan, write   (one small readback: the line count)
//   records:       parse per line, scan of the record and word counts
//                  (one small readback: the totals, the error word, the header's end)
//   emit:          records to their places, CIGAR words into the pool
//   one readback of [records | line numbers | pool]
//
// The workspace is the engine's own: grow-only buffers of the shared host layer
// (stage_host.hpp), released by hc_phmm_shutdown. A HIP error drains the stream
// before it returns. Calls serialise under the parser's own lock and use the
// engine's primary device. HC_SAM_TRACE=1 prints the host wall clock of the
// phases and the bytes moved on stderr; HC_SAM_STAGE_BYTES sizes the staging block.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hc_sam.h"
#include "sam_engine.hpp"
#include "sam_kernels.hpp"
#include "stage_host.hpp"

using namespace hcsam;
using namespace stage_host;

namespace {

Buf g_text, g_chunks, g_lines, g_out, g_stage{nullptr, 0, true}, g_hback{nullptr, 0, true}, g_hsmall{nullptr, 0, true};
Stage g_st({&g_text, &g_chunks, &g_lines, &g_out, &g_stage, &g_hback, &g_hsmall});

constexpr int64_t kMaxLines = 0x7f000000;   // below kNoHeaderEnd

size_t stage_bytes()
{
    const char* e = std::getenv("HC_SAM_STAGE_BYTES");
    const long long v = e ? std::atoll(e) : 0;
    return v >= 4096 ? size_t(v) : size_t(4) << 20;
}

const char* error_text(int64_t code)
{
    switch (code) {
        case kErrFields: return "fewer than 11 fields";
        case kErrFlag: return "FLAG is not a decimal number in 0 .. 65535";
        case kErrPos: return "POS is not a decimal number in 0 .. 4294967295";
        case kErrMapq: return "MAPQ is not a decimal number in 0 .. 65535";
        case kErrCigar: return "CIGAR is neither * nor elements of digits and one of MIDNSHP=X with lengths up to 268435455";
        case kErrPnext: return "PNEXT is not a decimal number in 0 .. 4294967295";
        case kErrTlen: return "TLEN is not a decimal number in -2147483648 .. 2147483647";
        case kErrLong: return "the line is longer than 2147483647 bytes";
        default: return "unknown device error";
    }
}

}  // namespace

stage_host::Stage& hcsam::parser_stage() { return g_st; }

int hcsam::upload(const uint8_t* bytes, int64_t len, size_t room, const uint8_t*& on_device)
{
    const Piece whole{bytes, len};
    return upload_pieces(&whole, 1, len, room, on_device);
}

int hcsam::upload_pieces(const Piece* pieces, size_t n_pieces, int64_t total, size_t room, const uint8_t*& on_device)
{
    const size_t stage = std::min(stage_bytes(), size_t(total));
    int rc = reserve(g_text, room, "SAM text on the device");
    if (rc) return rc;
    rc = reserve(g_stage, stage, "SAM text staging");
    if (rc) return rc;
    int64_t up = 0;    // bytes on the device
    size_t fill = 0;   // bytes in the block
    const auto flush = [&]() -> int {
        if (!fill) return HC_PHMM_OK;
        HIP_TRY(g_st.stream, hipMemcpyAsync(g_text.p + up, g_stage.p, fill, hipMemcpyHostToDevice, g_st.stream));
        HIP_TRY(g_st.stream, hipStreamSynchronize(g_st.stream));   // the block is reused by the next piece
        up += int64_t(fill);
        fill = 0;
        return HC_PHMM_OK;
    };
    for (size_t k = 0; k < n_pieces && stage; ++k) {
        for (int64_t off = 0; off < pieces[k].len && up + int64_t(fill) < total;) {   // never past `total` <= room
            const size_t n = size_t(std::min<int64_t>({int64_t(stage - fill), pieces[k].len - off, total - up - int64_t(fill)}));
            std::memcpy(g_stage.p + fill, pieces[k].bytes + off, n);
            fill += n;
            off += int64_t(n);
            if (fill == stage)
                if (int e = flush()) return e;
        }
    }
    if (int e = flush()) return e;
    on_device = reinterpret_cast<const uint8_t*>(g_text.p);
    return HC_PHMM_OK;
}

namespace {

int run(const uint8_t* text, int64_t len, hc_sam_result& res, Resident& dev)
{
    Trace tr("HC_SAM_TRACE", "[hc_sam]");
    SamArgs a{};
    a.len = len;
    a.n_chunks = (len + kChunkBytes - 1) / kChunkBytes;

    // ---- the text, through the staging block
    int rc = upload(text, len, size_t(a.n_chunks) * kChunkBytes, a.text);
    if (rc) return rc;
    rc = reserve(g_hsmall, 256, "SAM parser totals");
    if (rc) return rc;
    tr.mark("upload");

    // ---- line starts: count and scan
    Carver cc;
    const size_t o_cl = cc.take(sizeof(int32_t) * size_t(a.n_chunks));
    const size_t o_cf = cc.take(sizeof(int64_t) * (size_t(a.n_chunks) + 1));
    const size_t o_cw = cc.take(scan_work_bytes(a.n_chunks));
    rc = reserve(g_chunks, cc.off, "SAM parser chunk counts");
    if (rc) return rc;
    a.chunk_lines = reinterpret_cast<int32_t*>(g_chunks.p + o_cl);
    int64_t* chunk_first = reinterpret_cast<int64_t*>(g_chunks.p + o_cf);
    a.chunk_first = chunk_first;
    HIP_TRY(g_st.stream, launch_line_count(a, g_st.stream));
    HIP_TRY(g_st.stream, launch_scan(a.chunk_lines, a.n_chunks, chunk_first, reinterpret_cast<int64_t*>(g_chunks.p + o_cw), g_st.stream));
    int64_t* small = reinterpret_cast<int64_t*>(g_hsmall.p);
    HIP_TRY(g_st.stream, hipMemcpyAsync(small, chunk_first + a.n_chunks, sizeof(int64_t), hipMemcpyDeviceToHost, g_st.stream));
    HIP_TRY(g_st.stream, hipStreamSynchronize(g_st.stream));
    const int64_t n_lines = small[0];
    if (n_lines < 1 || n_lines > len) return fail(HC_PHMM_EHIP, "SAM parser: line count out of its bound");
    if (n_lines > kMaxLines) return fail(HC_PHMM_EINVAL, "more than " + std::to_string(kMaxLines) + " lines");
    a.n_lines = int32_t(n_lines);
    tr.mark("line_scan");

    // ---- per line: start, record slot, counts and their scans
    Carver lc;
    const size_t o_err = lc.take(sizeof(unsigned long long));
    const size_t o_he = lc.take(sizeof(int32_t));
    const size_t o_ls = lc.take(sizeof(int64_t) * size_t(n_lines));
    const size_t o_tmp = lc.take(sizeof(hc_sam_record) * size_t(n_lines));
    const size_t o_has = lc.take(sizeof(int32_t) * size_t(n_lines));
    const size_t o_nw = lc.take(sizeof(int32_t) * size_t(n_lines));
    const size_t o_rf = lc.take(sizeof(int64_t) * (size_t(n_lines) + 1));
    const size_t o_wf = lc.take(sizeof(int64_t) * (size_t(n_lines) + 1));
    const size_t o_lw = lc.take(scan_work_bytes(n_lines));
    rc = reserve(g_lines, lc.off, "SAM parser line workspace");
    if (rc) return rc;
    a.err = reinterpret_cast<unsigned long long*>(g_lines.p + o_err);
    a.header_end = reinterpret_cast<int32_t*>(g_lines.p + o_he);
    a.line_start = reinterpret_cast<int64_t*>(g_lines.p + o_ls);
    a.tmp = reinterpret_cast<hc_sam_record*>(g_lines.p + o_tmp);
    a.has_record = reinterpret_cast<int32_t*>(g_lines.p + o_has);
    a.n_words = reinterpret_cast<int32_t*>(g_lines.p + o_nw);
    int64_t* rec_first = reinterpret_cast<int64_t*>(g_lines.p + o_rf);
    int64_t* word_first = reinterpret_cast<int64_t*>(g_lines.p + o_wf);
    a.rec_first = rec_first;
    a.word_first = word_first;
    HIP_TRY(g_st.stream, hipMemsetAsync(a.err, 0xFF, sizeof(unsigned long long), g_st.stream));
    HIP_TRY(g_st.stream, hipMemsetAsync(a.header_end, 0x7F, sizeof(int32_t), g_st.stream));
    HIP_TRY(g_st.stream, launch_line_write(a, g_st.stream));
    HIP_TRY(g_st.stream, launch_parse(a, g_st.stream));
    int64_t* scan_work = reinterpret_cast<int64_t*>(g_lines.p + o_lw);   // the two scans run one after the other
    HIP_TRY(g_st.stream, launch_scan(a.has_record, n_lines, rec_first, scan_work, g_st.stream));
    HIP_TRY(g_st.stream, launch_scan(a.n_words, n_lines, word_first, scan_work, g_st.stream));
    HIP_TRY(g_st.stream, hipMemcpyAsync(small + 0, rec_first + n_lines, sizeof(int64_t), hipMemcpyDeviceToHost, g_st.stream));
    HIP_TRY(g_st.stream, hipMemcpyAsync(small + 1, word_first + n_lines, sizeof(int64_t), hipMemcpyDeviceToHost, g_st.stream));
    HIP_TRY(g_st.stream, hipMemcpyAsync(small + 2, a.err, sizeof(unsigned long long), hipMemcpyDeviceToHost, g_st.stream));
    HIP_TRY(g_st.stream, hipMemcpyAsync(small + 3, a.header_end, sizeof(int32_t), hipMemcpyDeviceToHost, g_st.stream));
    HIP_TRY(g_st.stream, hipStreamSynchronize(g_st.stream));
    const int64_t n_rec = small[0], n_words = small[1];
    unsigned long long err = 0;
    std::memcpy(&err, small + 2, sizeof(err));
    int32_t header_end = 0;
    std::memcpy(&header_end, small + 3, sizeof(header_end));
    tr.mark("parse");
    if (err != kNoError) {
        const int64_t line = int64_t(err >> 4);
        if (line >= n_lines) return fail(HC_PHMM_EHIP, "SAM parser: error word out of its bound");
        return fail(HC_PHMM_EINVAL, "line " + std::to_string(line + 1) + ": " + error_text(int64_t(err & 15ull)));
    }
    if (n_rec < 0 || n_rec > n_lines || n_words < 0) return fail(HC_PHMM_EHIP, "SAM parser: totals out of their bound");
    if (n_words > 0x7fffffffLL) return fail(HC_PHMM_EINVAL, "more than 2147483647 CIGAR elements");
    res.n_header_lines = header_end == kNoHeaderEnd ? int32_t(n_lines) : header_end;

    // ---- emit and read back
    Carver oc;
    const size_t o_rec = oc.take(sizeof(hc_sam_record) * size_t(n_rec));
    const size_t o_ln = oc.take(sizeof(int32_t) * size_t(n_rec));
    const size_t o_pool = oc.take(sizeof(uint32_t) * size_t(n_words));
    rc = reserve(g_out, oc.off, "SAM records on the device");
    if (rc) return rc;
    rc = reserve(g_hback, oc.off, "SAM records readback");
    if (rc) return rc;
    a.records = reinterpret_cast<hc_sam_record*>(g_out.p + o_rec);
    a.line_no = reinterpret_cast<int32_t*>(g_out.p + o_ln);
    a.pool = reinterpret_cast<uint32_t*>(g_out.p + o_pool);
    HIP_TRY(g_st.stream, launch_emit(a, g_st.stream));
    if (tr.on) {
        HIP_TRY(g_st.stream, hipStreamSynchronize(g_st.stream));
        tr.mark("emit");
    }
    HIP_TRY(g_st.stream, hipMemcpyAsync(g_hback.p, g_out.p, oc.off, hipMemcpyDeviceToHost, g_st.stream));
    HIP_TRY(g_st.stream, hipStreamSynchronize(g_st.stream));
    tr.mark("readback");
    const hc_sam_record* hr = reinterpret_cast<const hc_sam_record*>(g_hback.p + o_rec);
    const int32_t* hl = reinterpret_cast<const int32_t*>(g_hback.p + o_ln);
    const uint32_t* hp = reinterpret_cast<const uint32_t*>(g_hback.p + o_pool);
    res.records.assign(hr, hr + n_rec);   // one pass each: no zero fill in front of the copy
    res.line_no.assign(hl, hl + n_rec);
    res.pool.assign(hp, hp + n_words);
    tr.mark("records");
    tr.value("text_bytes", double(len));
    tr.value("lines", double(n_lines));
    tr.value("readback_bytes", double(oc.off));
    dev.stream = g_st.stream;
    dev.records = a.records;
    dev.line_no = a.line_no;
    dev.n_records = int32_t(n_rec);
    dev.text = a.text;
    dev.text_len = len;
    return HC_PHMM_OK;
}

}  // namespace

int hcsam::parse_resident(const uint8_t* text, int64_t text_len, hc_sam_result** out, std::unique_lock<std::mutex>& lk,
                          Resident& dev)
{
    std::unique_lock<std::mutex> mine(g_st.mu);
    dev = Resident{};
    const int rc = call_frame(out, &g_st.stream, [&](hc_sam_result& res) -> int {
        if (text_len < 0 || (text_len && !text)) return fail(HC_PHMM_EINVAL, "null text / negative length");
        if (int rc = g_st.ensure_init()) return rc;
        dev.stream = g_st.stream;
        return text_len ? run(text, text_len, res, dev) : HC_PHMM_OK;
    });
    if (!rc) lk = std::move(mine);
    return rc;
}

extern "C" int hc_sam_parse(const uint8_t* text, int64_t text_len, hc_sam_result** out)
{
    std::unique_lock<std::mutex> lk;
    Resident dev;
    return parse_resident(text, text_len, out, lk, dev);
}

extern "C" int hc_sam_result_records(const hc_sam_result* res, const hc_sam_record** records, const int32_t** line_no,
                                     int32_t* n_records, const uint32_t** cigar_pool, int32_t* n_words,
                                     int32_t* n_header_lines)
{
    if (!res) return fail(HC_PHMM_EINVAL, "null result");
    if (records) *records = res->records.data();
    if (line_no) *line_no = res->line_no.data();
    if (n_records) *n_records = int32_t(res->records.size());
    if (cigar_pool) *cigar_pool = res->pool.data();
    if (n_words) *n_words = int32_t(res->pool.size());
    if (n_header_lines) *n_header_lines = res->n_header_lines;
    return HC_PHMM_OK;
}

extern "C" int hc_sam_result_free(hc_sam_result* res)
{
    delete res;
    return HC_PHMM_OK;
}
