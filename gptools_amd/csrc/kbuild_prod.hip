// kbuild_prod.hip -- the PRODUCT of two native kernels (GPT_KERNEL_PRODUCT / GPT_KID_PRODUCT_GM, kpair.hpp prod_pair; ref:
// gptools/kernel/core.py:587-671) in the single-matrix builder and the pair list: the same kernels and the same host dispatch as
// kbuild.hip (kbuild_kernel.hpp), for the list ProductKids -- once per num_dim, the factors chosen at run time.  Nothing but the two
// calls that instantiate them: a translation unit of its own so that they compile beside the others.
#include "kbuild_kernel.hpp"

int kbuild_prod(hipStream_t st, const KParams &kp1, const KParams &kp2, const KBuildArgs &a)
{
    return kbuild_dispatch(ProductKids(), product_kid(kp1.D, gibbs_form_of(kp1.D, kp1.kernel_id, kp2.kernel_id), gibbs_more_kid(kp1.kernel_id) || gibbs_more_kid(kp2.kernel_id), false), st, kp1, kp2, a);
}

int kpairs_prod(hipStream_t st, const KParams &kp1, const KParams &kp2, const KPairsArgs &a)
{
    return kpairs_dispatch(ProductKids(), product_kid(kp1.D, gibbs_form_of(kp1.D, kp1.kernel_id, kp2.kernel_id), gibbs_more_kid(kp1.kernel_id) || gibbs_more_kid(kp2.kernel_id), false), st, kp1, kp2, a);
}
