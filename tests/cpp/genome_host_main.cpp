// Host program for tests/test_genome_host.py: csrc/genome_body.hpp compiled for
// the host (SAMX_HOST_ONLY) and run on one thread under
// -fsanitize=address,undefined. genome_resolve_kernel makes a row's "not
// whitespace" mask by a wave ballot; here a loop over the 64 bytes makes it.
// Everything else is genome_body.hpp's own text: the third token, the hash, the
// probe, the compare and the window-to-contig search. The text, the name pool,
// the name offsets, the slots and the window sums live in heap blocks of
// exactly their sizes, so a read past them is an error, not a silent success.
//
//   genome_host_main IN.sam TABLE REGION OUT
//
// TABLE: one line "name ref_len" per contig, in table order.
// OUT:   "R n" and one line "line_offset contig_of" per line of IN that does
//        not begin with '@' (the test feeds it texts in which every such line
//        is a record, as the kernel is given records only), then "W n" and the
//        contig of every genome-wide window, one per line, then "P n": the
//        names that did not get their hash's own slot.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "../../gatk-haplotypecaller-cpp17_amd/csrc/genome_body.hpp"

using namespace hcgenome;

static uint64_t row_mask(const uint8_t* t, int64_t at, int64_t end)
{
    uint64_t m = 0;
    for (int l = 0; l < 64 && at + l < end; ++l)
        if (!hcsam::sam_space(t[at + l])) m |= uint64_t(1) << l;
    return m;
}

// genome_resolve_kernel's work on the line that begins at `begin`; -2 for a line without a third token.
static int32_t resolve(const uint8_t* t, int64_t len, int64_t begin, const GenomeTable& table)
{
    GenomeRname tk;
    for (int64_t off = 0; begin + off < len && !tk.done(); off += 64) tk.row(row_mask(t, begin + off, len), off);
    if (!tk.done()) return -2;
    if (tk.end - tk.begin > 255) return -1;
    uint32_t slot;
    return genome_lookup(table, t + begin + tk.begin, tk.end - tk.begin, slot);
}

int main(int argc, char** argv)
{
    if (argc != 5) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    std::ifstream tab(argv[2]);
    if (!in || !tab) return 2;
    const int64_t region = std::atoll(argv[3]);
    const std::string whole((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const int64_t len = int64_t(whole.size());
    std::unique_ptr<uint8_t[]> text(new uint8_t[size_t(len)]);   // no terminator, no slack
    std::memcpy(text.get(), whole.data(), size_t(len));

    std::vector<std::string> names;
    std::vector<int64_t> lens;
    std::string name;
    int64_t n_bases = 0;
    while (tab >> name >> n_bases) {
        names.push_back(name);
        lens.push_back(n_bases);
    }
    const int32_t n = int32_t(names.size());
    if (n < 1 || region < 1) return 2;
    size_t pool_bytes = 0;
    for (const std::string& s : names) pool_bytes += s.size();
    const uint32_t n_slots = genome_table_slots(n);
    std::unique_ptr<uint8_t[]> pool(new uint8_t[pool_bytes]);
    std::unique_ptr<int32_t[]> name_off(new int32_t[size_t(n) + 1]);
    std::unique_ptr<int32_t[]> slots(new int32_t[n_slots]);
    std::unique_ptr<int64_t[]> win_off(new int64_t[size_t(n) + 1]);
    for (uint32_t s = 0; s < n_slots; ++s) slots[s] = -1;
    const GenomeTable table{slots.get(), n_slots - 1u, name_off.get(), pool.get()};
    name_off[0] = 0;
    win_off[0] = 0;
    int64_t probes_past_first = 0;
    for (int32_t k = 0; k < n; ++k) {   // as genome_engine.cpp builds it
        const uint8_t* s = reinterpret_cast<const uint8_t*>(names[size_t(k)].data());
        const int64_t sn = int64_t(names[size_t(k)].size());
        uint32_t slot = 0;
        if (genome_lookup(table, s, sn, slot) >= 0) return 4;   // two equal names
        if (slot != (genome_hash(s, sn) & table.mask)) ++probes_past_first;
        std::memcpy(pool.get() + name_off[k], s, size_t(sn));
        name_off[k + 1] = name_off[k] + int32_t(sn);
        slots[slot] = k;
        win_off[k + 1] = win_off[k] + (lens[size_t(k)] + region - 1) / region;
    }

    std::ofstream out(argv[4]);
    std::vector<std::pair<int64_t, int32_t>> rows;
    for (int64_t i = 0; i < len; ++i) {
        if (i != 0 && text[size_t(i - 1)] != '\n') continue;
        if (text[size_t(i)] == '@') continue;
        const int32_t c = resolve(text.get(), len, i, table);
        if (c != -2) rows.emplace_back(i, c);
    }
    out << "R " << rows.size() << '\n';
    for (const auto& r : rows) out << r.first << ' ' << r.second << '\n';
    out << "W " << win_off[n] << '\n';
    for (int64_t w = 0; w < win_off[n]; ++w) out << genome_contig_of_window(win_off.get(), n, w) << '\n';
    out << "P " << probes_past_first << '\n';
    return 0;
}
