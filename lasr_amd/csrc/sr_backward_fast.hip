// sr_backward_fast.hip -- backward raster kernel for LASR's mode combination (euclidean / softmax / prod / vertex attributes /
// double sided), 3, 6 and 9 attribute channels.  Same template as the generic instantiation in sr_raster.hip (sr_backward.h),
// but THIS translation unit is compiled with -ffp-contract=fast-honor-pragmas (see the Makefile): the backward pass is VALU-issue bound and
// its gradient bar is relative 1e-3, so v_mul_f32 + v_add_f32 pairs fuse into v_fma_f32.
#include <hip/hip_runtime.h>

#include "sr_backward.h"

namespace lasr {

void launch_backward_fast(int nch, dim3 grid, hipStream_t st, const RasterArgs& A, const float* colors, const float* aggrs,
                          const float* gcolors, float* gfaces, float* gtex)
{
    // (A.plane_off32: the plan's decision whether the pixel planes' byte offsets fit 32 bits, sr_common.h)
#define LASR_LAUNCH_BWD(NCH, WIDE) \
    hipLaunchKernelGGL((sr_backward_kernel<true, NCH, WIDE>), grid, dim3(BWD_THREADS), 0, st, A, colors, aggrs, gcolors, gfaces, gtex)
    if (nch == 9) { if (A.plane_off32) LASR_LAUNCH_BWD(9, false); else LASR_LAUNCH_BWD(9, true); }
    else if (nch == 6) { if (A.plane_off32) LASR_LAUNCH_BWD(6, false); else LASR_LAUNCH_BWD(6, true); }
    else { if (A.plane_off32) LASR_LAUNCH_BWD(3, false); else LASR_LAUNCH_BWD(3, true); }
#undef LASR_LAUNCH_BWD
}

}  // namespace lasr
