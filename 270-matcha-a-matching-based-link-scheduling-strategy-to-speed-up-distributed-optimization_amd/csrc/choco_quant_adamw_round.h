// choco_quant_adamw_round.h -- torch.optim.AdamW's (decoupled = 0: Adam's) step as a step policy of
// choco_quant_round.h's quant_round: what choco_quant_adamw_round.hip (fp32 models) and
// choco_quant_adamw_round_bf16.hip (bfloat16 models and gradients over fp32 x, x_hat, s, exp_avg and exp_avg_sq)
// share; the design is at the head of the former.  The update is adam_update.h's adam4: x, x_hat, s and the norms
// are the bits of mx_choco_quant_round on x' = adam(x, g, m, v), m' and v' the bits of the fused AdamW rounds.
#pragma once
#include "adam_update.h"
#include "choco_quant_round.h"

namespace mx {
namespace choco {
namespace qround {
using mx::fused::AdamHyper;
using mx::fused::AdamState;

// g, m and v of a lane's four columns STREAM through two lanes, dead once m', v' and the zeros are stored: only x
// and x_hat of a wave's four items are in flight at once (the head of choco_quant_adamw_round.hip says why)
struct AdamStep : StepBase {
    using Hyper = AdamHyper;
    using State = AdamState;
    template <class IO>
    struct Stream {
        typename IO::GC g;
        F4 m, v;
    };
    static constexpr bool kSteps = true;
    static __device__ __forceinline__ bool no_step(State& st, const Hyper& h) { return mx::fused::adam_no_step(st, h); }
    static __device__ __forceinline__ void setup(State& st, const Hyper& h) { mx::fused::adam_setup(st, h); }
    template <class IO>
    static __device__ __forceinline__ bool al(bool base, const typename IO::GT* g, const float* m, const float* v,
                                              int64_t off) {
        return base && al16(m + off) && al16(v + off) && IO::al_g(g + off);
    }
    template <class IO, bool NT>
    static __device__ __forceinline__ Stream<IO> load(const typename IO::GT* g, const float* m, const float* v,
                                                      int64_t off, int64_t c, bool vec, int64_t P) {
        Stream<IO> ln;
        ln.g = load_q<NT>(g + off, c, vec, P);
        ln.m = load_q<NT>(m + off, c, vec, P);
        ln.v = load_q<NT>(v + off, c, vec, P);
        return ln;
    }
    template <class IO, bool NT>
    static __device__ __forceinline__ void step(F4& xv, None&, int, Stream<IO>& ln, const State& st, const Hyper& h,
                                                typename IO::GT* g, float* m, float* v, int64_t off, int64_t c,
                                                bool vec, int64_t P) {
        xv = mx::fused::adam4(xv, mx::fused::widen4(ln.g), ln.m, ln.v, st.st, h);
        store_q<NT>(ln.m, m + off, c, vec, P);
        store_q<NT>(ln.v, v + off, c, vec, P);
        if (h.zero_grads) store_q<NT>(IO::zero(), g + off, c, vec, P);
    }
    static bool given(const Hyper& h, const void* g, const float* m, const float* v) { return g && m && v && h.bias; }
    static int check(const char* who, const Hyper& h, const float*, const float*) {
        MX_CHECK(h.n_bias >= 1, "%s: n_bias=%lld < 1", who, (long long)h.n_bias);
        MX_CHECK(h.step_dev || h.step >= 1, "%s: optimizer step %lld < 1", who, (long long)h.step);
        return MX_OK;
    }
    template <class IO, class... F>
    static auto kernel(const Hyper&, int bits, bool nt) { return pick<IO, AdamStep, F...>(bits, nt); }
};

// the entry points' arguments as the step's constants
inline AdamHyper adam_hyper(float lr, const float* lr_dev, float omb1, float beta2, float omb2, float eps, float wd,
                            int decoupled, int zero_grads, const float* bias_dev, int64_t n_bias, int64_t step,
                            const int64_t* step_dev) {
    return {lr, wd, omb1, beta2, omb2, eps, lr_dev, nullptr, bias_dev, n_bias, step, step_dev, decoupled != 0,
            zero_grads != 0};
}

}  // namespace qround
}  // namespace choco
}  // namespace mx
