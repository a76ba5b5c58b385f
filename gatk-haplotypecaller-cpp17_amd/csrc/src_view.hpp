// Where a call's reads and haps live, as the engine's host passes see them
// (engine_core.hpp includes this; flat_records.hpp needs nothing else of it).
#pragma once
#include <cstdint>

#include "../../include/hc_pairhmm.h"

namespace hcphmm {
namespace eng {

struct ReadView {
    int32_t len;
    const uint8_t *bases, *q, *i, *d, *c;
};
struct HapView {
    int32_t len;
    const uint8_t* bases;
};

// Where a call's reads and haps live: flat pools (pair p = read p x hap p) or
// struct arrays (hc_phmm_read / hc_phmm_hap).
struct Src {
    const int64_t* read_off = nullptr;
    const int32_t* R = nullptr;
    const int64_t* hap_off = nullptr;
    const int32_t* H = nullptr;
    const uint8_t *rs = nullptr, *q = nullptr, *ins = nullptr, *del = nullptr, *gcp = nullptr, *hap = nullptr;
    const hc_phmm_read* reads = nullptr;
    const hc_phmm_hap* haps = nullptr;

    ReadView read(int64_t k) const
    {
        if (reads) {
            const hc_phmm_read& r = reads[k];
            return ReadView{r.length, (const uint8_t*)r.bases, (const uint8_t*)r.q, (const uint8_t*)r.i,
                            (const uint8_t*)r.d, (const uint8_t*)r.c};
        }
        const int64_t o = read_off[k];
        return ReadView{R[k], rs + o, q + o, ins + o, del + o, gcp + o};
    }
    HapView hapv(int64_t k) const
    {
        if (haps) return HapView{haps[k].length, (const uint8_t*)haps[k].bases};
        return HapView{H[k], hap + hap_off[k]};
    }
    int32_t read_len(int64_t k) const { return reads ? reads[k].length : R[k]; }
    int32_t hap_len(int64_t k) const { return haps ? haps[k].length : H[k]; }
};

// The one way to build a flat Src (the pools of hc_phmm_pairs_flat's arguments).
inline Src flat_src(const int64_t* read_off, const int32_t* R, const int64_t* hap_off, const int32_t* H,
                    const uint8_t* rs, const uint8_t* q, const uint8_t* ins, const uint8_t* del, const uint8_t* gcp,
                    const uint8_t* hap)
{
    Src s;
    s.read_off = read_off;
    s.R = R;
    s.hap_off = hap_off;
    s.H = H;
    s.rs = rs;
    s.q = q;
    s.ins = ins;
    s.del = del;
    s.gcp = gcp;
    s.hap = hap;
    return s;
}

}  // namespace eng
}  // namespace hcphmm
