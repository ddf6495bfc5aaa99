// Which instantiation of the resident B-grid kernel a launch runs (evp_device.h: Res2Facts)
#include "evp_device.h"

Res2Choice res2_choose(const Res2Facts &f)
{
    const bool tile16 = f.logw == 4 && !f.rimg;
    // rim T-cells by corners (COOP): built, every tile's rim list fits its 64 quads, the chip takes all tiles with its larger LDS share
    const bool coop = f.want_coop && f.coop_ok && tile16 && !f.remote && f.coop_built && f.coop_fits;
    // the lean variant where nothing it leaves out can happen in this launch
    const bool lean = !coop && f.want_lean && f.cap == 3 && tile16 && f.nblocks == 1 && !f.seam && !f.tfold && !f.img3 && !f.rraw &&
                      f.revp_zero && (f.flags & EVP_F_WATER_IS_OCN) && (f.flags & EVP_F_TBU_ZERO);
    // ... on the rim-wave schedule where every tile's lane tables satisfy its rules
    const bool rimu = lean && f.want_rimu && f.rimu_ok && !(f.hooks & EVP_RES2_HOOK_BARS_RIMU);
    return {{f.strict, f.cap, f.logw, f.rimg, coop, lean, rimu}, rimu};
}
