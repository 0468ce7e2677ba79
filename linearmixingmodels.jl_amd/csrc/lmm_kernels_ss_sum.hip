// lmm_kernels_ss_sum.hip -- the state-space kernels of lmm_kernels_ss.h instantiated for the sums of two terms inside one latent
// (DESIGN.md 4.18 "Sum latents"): the seven pair models SS_PAIR(a, b), D = D_a + D_b <= 4.  A translation unit of its own because these
// instantiations take more than twice the compile time of the one-term models; built like lmm_kernels_ss.hip, WITHOUT
// -amdgpu-mfma-vgpr-form=1 (no MFMA here).  No kernel text: lmm_kernels_ss.hip's launch_ss_* come here for a sum's model.
#include "lmm_kernels_ss.h"

namespace {

struct SSPairModels {
  template <typename F>
  static auto dispatch(int model, F&& f) {
    if (model == SS_PAIR(1, 1)) return f(SSPairTag<1, 1>());
    if (model == SS_PAIR(1, 2)) return f(SSPairTag<1, 2>());
    if (model == SS_PAIR(1, SS_MODEL_SHO)) return f(SSPairTag<1, SS_MODEL_SHO>());
    if (model == SS_PAIR(1, 3)) return f(SSPairTag<1, 3>());
    if (model == SS_PAIR(2, 2)) return f(SSPairTag<2, 2>());
    if (model == SS_PAIR(2, SS_MODEL_SHO)) return f(SSPairTag<2, SS_MODEL_SHO>());
    return f(SSPairTag<SS_MODEL_SHO, SS_MODEL_SHO>());
  }
};

}  // namespace

void launch_ss_filter_pair(const SSArgs& a, int model, int nb, double* lml, hipStream_t st) { ss_launch_filter<SSPairModels>(a, model, nb, lml, st); }
void launch_ss_smooth_pair(const SSArgs& a, int model, int nb, hipStream_t st) { ss_launch_smooth<SSPairModels>(a, model, nb, st); }
void launch_ss_filter_from_pair(const SSFromArgs& a, int model, int nb, double* lml, hipStream_t st) { ss_launch_filter_from<SSPairModels>(a, model, nb, lml, st); }
void launch_ss_smooth_kept_pair(const SSArgs& a, int model, int nb, hipStream_t st) { ss_launch_smooth_kept<SSPairModels>(a, model, nb, st); }
void launch_ss_grad_pair(const SSArgs& a, int model, int nb, double* gtheta, hipStream_t st) { ss_launch_grad<SSPairModels>(a, model, nb, gtheta, st); }
void launch_ss_path_pair(const SSPathArgs& a, int model, int nb, hipStream_t st) { ss_launch_path<SSPairModels>(a, model, nb, st); }
void launch_ss_post_path_pair(const SSPostArgs& a, int model, int nb, hipStream_t st) { ss_launch_post_path<SSPairModels>(a, model, nb, st); }
void launch_ss_post_logpdf_pair(const SSLpdfArgs& a, int model, int nb, double* lml, hipStream_t st) { ss_launch_post_logpdf<SSPairModels>(a, model, nb, lml, st); }
void launch_ss_interp_pair(const SSInterpArgs& a, int model, int nb, hipStream_t st) { ss_launch_interp<SSPairModels>(a, model, nb, st); }
