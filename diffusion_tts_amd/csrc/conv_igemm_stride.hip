// The stride-2 forms of conv_igemm_kernel (S2 = true: the 3x3 convolution with zero padding 1 and stride 2 in the 16-bit modes,
// dts_conv_args.up == -1 -- the SD U-Net's Downsample2D without a space-to-depth pass) as a translation unit of their own: conv_igemm.hip
// without its C entry points, with dts_conv_launch_stride_form() and the 24 kernels it names (f16 | bf16, cout tile 64 | 128 | 192, 4 | 8 waves,
// 2- | 3-deep ring).  Compiled in parallel with conv_igemm.hip, the longest compile of the build, whose own kernels it leaves as they were.
#define DTS_CONV_STRIDE_TU
#include "conv_igemm.hip"
