// k_polar_mx (k_polar_mx.hiph): the instances specialised for the shape of an HDR10 -> SDR map chain
#include "k_polar_mx.hiph"

int plh_launch_polar_mx_shape(hipStream_t stream, const plh_pass *pass, int shape)
{
    switch (shape) {
    case PLH_SHAPE_BT1886:  return launch_mx_variant<3, true, MX_POST_SHAPE + 0, 8>(stream, pass);
    case PLH_SHAPE_GAMMA:   return launch_mx_variant<3, true, MX_POST_SHAPE + 1, 8>(stream, pass);
    case PLH_SHAPE_SRGB:    return launch_mx_variant<3, true, MX_POST_SHAPE + 2, 8>(stream, pass);
    }
    return 1;
}
