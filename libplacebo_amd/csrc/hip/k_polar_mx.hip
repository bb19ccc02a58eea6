// k_polar_mx instantiations (k_polar_mx.hiph): RGB and RGBA tiles
#include "k_polar_mx.hiph"

// an exact 2x upscale of an RGB or RGBA tile: every op shape has an instance (launch_mx)
bool plh_polar_mx_applies(plh_pass *pass)
{
    const uint32_t cm = pass->s.comp_mask & 0xf;
    if (!pass->s.pp || pass->s.mx.enabled != 1 || (cm != 0x7 && cm != 0xf))
        return false;
    // (the kernel has a variant for the map chain of an HDR pass, contrast recovery included: RGB tiles)
    if (cm == 0x7)
        plh_match_map_chain(pass, true);
    if (!pass->chain.enabled)
        plh_match_fast_epilogue(pass);
    return true;
}

int plh_launch_polar_mx(hipStream_t stream, const plh_pass *pass)
{
    return (pass->s.comp_mask & 0xf) == 0x7 ? launch_mx<3>(stream, pass) : launch_mx<4>(stream, pass);
}
