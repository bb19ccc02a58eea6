// k_polar_mx (k_polar_mx.hiph): the instances specialised for the shape of an HDR10 -> SDR map chain
#include "k_polar_mx.hiph"

template <int POST>
static int launch_shape(hipStream_t stream, const plh_pass *pass)
{
    if (!launch_mx_variant<3, true, POST, 8>(stream, pass))
        return 1;
    return plh_launch_status();
}

int plh_launch_polar_mx_shape(hipStream_t stream, const plh_pass *pass, int shape)
{
    switch (shape) {
    case PLH_SHAPE_BT1886:  return launch_shape<MX_POST_SHAPE + 0>(stream, pass);
    case PLH_SHAPE_GAMMA:   return launch_shape<MX_POST_SHAPE + 1>(stream, pass);
    case PLH_SHAPE_SRGB:    return launch_shape<MX_POST_SHAPE + 2>(stream, pass);
    }
    return 1;
}
