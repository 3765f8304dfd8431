// The phase forms of conv_igemm_kernel (PH = true: a nearest-2x upsampled 3x3 convolution in split precision as four 2x2 convolutions over the
// low-resolution input, dts_conv_args.up == 2) as a translation unit of their own: conv_igemm.hip without its C entry points, with
// dts_conv_launch_phase_form() and the eight kernels it names.  Compiled in parallel with conv_igemm.hip, the longest compile of the build.
#define DTS_CONV_PHASE_TU
#include "conv_igemm.hip"
