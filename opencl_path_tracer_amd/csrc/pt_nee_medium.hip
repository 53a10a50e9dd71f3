// pt_nee_medium.hip -- the medium instances of k_nee (k_nee<kNeeMedium, ...>; pt_set_medium) and their launcher,
// launch_nee_tu<kNeeMedium>: pt_nee.hip's one body, nee_frame, instantiated for the family in a translation unit of its own, so that the other
// families' instances compile exactly as they did before these existed (see launch_nee_tu there).
#define PT_NEE_TU PT_NEE_FAMILY_MEDIUM
#include "pt_nee.hip"
