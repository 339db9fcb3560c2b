// mt_apply_locw.hip -- the LDS engine's wide editing form (include/mtgpu.h "limits": an editing client's
// document past the narrow limits): mt::apply_kernel_g<CAP, /*W*/ true, /*LOC*/ true, GW> at 1024 / 4096 /
// 8192 slots, GW = 1 and MT_LOC_GW, and their launcher (mt_launch_apply_loc_wide).  The engine itself is
// mt_apply.hip's; this translation unit instantiates only these six kernels, so they compile in
// parallel with the rest of the engine.
#define MT_APPLY_LOCW_TU
#include "mt_apply.hip"
