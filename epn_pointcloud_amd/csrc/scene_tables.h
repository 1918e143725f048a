// The host-side check of a scene's tables (include/epn_so3conv.h, "Scene tables"), shared by the entries that take them:
// descriptor matching (desc_match.hip) and pairwise registration (ransac_register.hip).  Reads host memory only.
#pragma once
#include <stdint.h>

#include "../../include/epn_so3conv.h"

namespace epn {

constexpr int SCENE_MAX_PAIRS = 32767;   // a grid dimension of 2 P in the nearest-neighbour kernel

// The scene's tables, from the caller's HOST copies: frag_off ascending from 0 to R with fragments of fewer than 2^31 rows,
// pairs inside 0..F-1 with src != tgt, out_off and tgt_off (each checked if given) equal to their formulas.  *max_rows: the
// largest fragment a pair uses.  need_out: out_off is a required table of the calling entry.
inline int check_scene(int64_t R, int F, const int64_t *frag_off, int P, const int32_t *pairs, const int64_t *out_off,
                       const int64_t *tgt_off, int64_t *max_rows, bool need_out = true) {
    if (R < 0 || F < 1 || P < 0 || P > SCENE_MAX_PAIRS) return EPN_EINVAL;
    if (!frag_off || (need_out && !out_off) || (P > 0 && !pairs)) return EPN_ENULL;
    if (frag_off[0] != 0 || frag_off[F] != R) return EPN_EINVAL;
    for (int f = 0; f < F; ++f)
        if (frag_off[f + 1] < frag_off[f] || frag_off[f + 1] - frag_off[f] > (int64_t)INT32_MAX) return EPN_EINVAL;
    int64_t o = 0, t = 0, m = 0;
    if ((out_off && out_off[0] != 0) || (tgt_off && tgt_off[0] != 0)) return EPN_EINVAL;
    for (int p = 0; p < P; ++p) {
        const int32_t s = pairs[2 * p], d = pairs[2 * p + 1];
        if (s < 0 || s >= F || d < 0 || d >= F || s == d) return EPN_EINVAL;
        const int64_t ns = frag_off[s + 1] - frag_off[s], nt = frag_off[d + 1] - frag_off[d];
        o += ns + nt;
        t += nt;
        if ((out_off && out_off[p + 1] != o) || (tgt_off && tgt_off[p + 1] != t)) return EPN_EINVAL;
        m = ns > m ? ns : m;
        m = nt > m ? nt : m;
    }
    *max_rows = m;
    return 0;
}

}  // namespace epn
