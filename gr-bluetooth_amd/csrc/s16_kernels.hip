// s16_kernels.hip -- the int16-input kernels' own translation unit: the explicit instantiations s16_inst.h lists, which
// btgpu.hip declares extern.  Built with libbtgpu.so's own flags (Makefile), so that the arithmetic behind the widening loads
// is compiled as in the float-input forms and gives the same bits.
#define BTGPU_S16_INSTANTIATE
#include "s16_inst.h"
