// What the genome caller (include/hc_genome.h) decides per record and per
// window, written once for the device and the host: the RNAME of an alignment
// line (its third token, found from the "not whitespace" masks of sam_body.hpp
// row by row), the hash of a name, the probe of the contig table with the
// compare that confirms a hit, and the contig of a genome-wide window.
// genome_kernels.hip makes a row's mask by a wave ballot; with SAMX_HOST_ONLY
// (no HIP header) tests/cpp/genome_host_main.cpp makes it with a loop over 64
// bytes and runs the same functions under the host sanitizers. No byte at or
// past the text's length, the pool's length or the table's size is read.
//
// The table. Open addressing with linear probing over `mask + 1` slots, a power
// of two of at least twice the contig count, so a probe always meets an empty
// slot (-1). A slot holds a contig index; contig c's name is the bytes
// pool[name_off[c], name_off[c + 1]). A slot whose name has another length or
// other bytes is passed over: two names with one hash, or one name a prefix of
// another, are different names.
#pragma once
#include "sam_body.hpp"

namespace hcgenome {

// FNV-1a, 32 bits.
SAMX_FN inline uint32_t genome_hash(const uint8_t* s, int64_t n)
{
    uint32_t h = 2166136261u;
    for (int64_t i = 0; i < n; ++i) h = (h ^ uint32_t(s[i])) * 16777619u;
    return h;
}

struct GenomeTable {
    const int32_t* slots;     // mask + 1 entries: a contig index or -1
    uint32_t mask;
    const int32_t* name_off;  // n_contigs + 1
    const uint8_t* pool;      // name_off[n_contigs] bytes
};

// The smallest power of two that is at least twice n (n >= 1).
SAMX_FN inline uint32_t genome_table_slots(int32_t n)
{
    uint32_t s = 2;
    while (s < 2u * uint32_t(n)) s <<= 1;
    return s;
}

SAMX_FN inline bool genome_same(const GenomeTable& t, int32_t c, const uint8_t* s, int64_t n)
{
    const int32_t b = t.name_off[c];
    if (int64_t(t.name_off[c + 1] - b) != n) return false;
    for (int64_t i = 0; i < n; ++i)
        if (t.pool[b + i] != s[i]) return false;
    return true;
}

// The contig named s[0, n), or -1. `slot` gets where the probe ended: the hit,
// or the empty slot a new name would take.
SAMX_FN inline int32_t genome_lookup(const GenomeTable& t, const uint8_t* s, int64_t n, uint32_t& slot)
{
    for (slot = genome_hash(s, n) & t.mask;; slot = (slot + 1u) & t.mask) {
        const int32_t c = t.slots[slot];
        if (c < 0 || genome_same(t, c, s, n)) return c;
    }
}

// The third token of a line, fed row by row as SamTokens is: `begin` and `end`
// are offsets from the line's first byte once done(). A line that has a record
// has eleven tokens, so its third one ends before the line does.
struct GenomeRname {
    int32_t n_start = 0, n_end = 0;
    int64_t begin = 0, end = 0;
    uint64_t carry = 0;
    SAMX_FN bool done() const { return n_end >= 3; }
    SAMX_FN void row(uint64_t nonws, int64_t off)
    {
        uint64_t starts, ends;
        hcsam::sam_token_masks(nonws, carry, starts, ends);
        carry = nonws >> 63;
        for (; starts && n_start < 3; starts &= starts - 1)
            if (++n_start == 3) begin = off + hcsam::sam_ctz(starts);
        for (; ends && n_end < 3; ends &= ends - 1)
            if (++n_end == 3) end = off + hcsam::sam_ctz(ends);
    }
};

// Contig c's windows are [win_off[c], win_off[c + 1]); every contig has at least
// one, so the contig of window w (0 <= w < win_off[n_contigs]) is the last c
// with win_off[c] <= w.
SAMX_FN inline int32_t genome_contig_of_window(const int64_t* win_off, int32_t n_contigs, int64_t w)
{
    int32_t lo = 0, hi = n_contigs - 1;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (win_off[mid] <= w)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// A read of contig c (-1: none) with 1-based POS lies in the contig.
SAMX_FN inline bool genome_placed(int32_t c, uint32_t pos, const int64_t* ref_len)
{
    return c >= 0 && pos != 0u && int64_t(pos - 1u) < ref_len[c];
}

}  // namespace hcgenome
