// s8_kernels.hip -- the int8-input kernels' own translation unit: the explicit instantiations s8_inst.h lists, which
// btgpu.hip declares extern.  Built with libbtgpu.so's own flags (Makefile), so that the arithmetic behind the widening loads
// is compiled as in the float-input forms and gives the same bits.
#define BTGPU_S8_INSTANTIATE
#include "s8_inst.h"
