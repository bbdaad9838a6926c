// sample_con.hip -- the CONSTRAINED form of the sampling finish (kernels.h: ConFinishParams; include/emmax.h: emmax_session_set_automaton):
// emmax_sample_kernel<ConFinishParams> of sample_kernel.h and its launcher.
//
// A translation unit of its own, on purpose.  As a sixth instantiation beside sample.hip's five it changed what the inliner did to them (in the
// EXT finish process_row, the top-p radix walk and block_argmax became calls, and its scratch and spill figures moved), and a session that sets
// no automaton is to launch the code it launched before.  Here sample.hip's object keeps its kernels instruction for instruction
// (profiles/constraint_isa_unchanged.txt), and this one holds the constrained kernel alone.
#include "sample_kernel.h"

int launch_con_finish(const ConFinishParams& p, hipStream_t stream) {
    if (p.f.B < 1 || p.V < 1 || p.V > EMMAX_SAMPLE_MAX_V || p.ld < p.V) return -1;
    if (!p.penalty || !p.ngram || !p.min_new || !p.hist || !p.hist_len || p.max_prompt < 1) return -1;   // the mask is one of the processors
    if (p.rt.off && (!p.rt.ids || !p.rt.flags || !p.rt.bias || !p.rule_en || (!p.rt.n && (p.rt.n_host < 0 || p.rt.n_host > EMMAX_MAX_RULES)))) return -1;
    if (p.min_p && (!p.typical_p || !p.eps_cut || !p.eta_cut)) return -1;
    if (p.tok_out && (!p.logprob_out || !p.f.is_prefill || p.f.max_out != 0)) return -1;
    if (!p.cls || !p.allow || !p.next || !p.state || p.n_states < 1 || p.n_states > EMMAX_MAX_AUT_STATES || p.next_ld < 1 || p.next_ld > EMMAX_MAX_AUT_CLASSES) return -1;
    hipLaunchKernelGGL(emmax_sample_kernel<ConFinishParams>, dim3(p.f.B), dim3(ST), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
