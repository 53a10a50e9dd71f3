// pt_nee_medium.hip -- the medium instances of k_nee (k_nee_medium, k_nee_env_medium, k_nee_tiles_medium, k_nee_env_tiles_medium; pt_set_medium,
// DESIGN.md section 5.17) and their launcher, launch_nee_medium: pt_nee.hip's one body, nee_frame, instantiated with MEDIUM in a translation
// unit of its own, so that the other families' instances compile exactly as they did before these existed (see launch_nee_medium there).
#define PT_NEE_MEDIUM_TU 1
#include "pt_nee.hip"
