// model.hip -- the model half of the host side of libemmax_hip.so: the tuning table, weight binding + re-layout into the arenas
// (finalize, build_aux) and the emmax_model_* / emmax_tuning_* part of the C ABI of include/emmax.h.  The session and the stages that
// run on it are in session / vision / prefill / step / generate / modes / ops .hip (session.h).  No device code lives here; kernels
// are in gemm / norm / attention / misc / decode .hip.
#include <array>
#include <cctype>
#include <cstdarg>
#include <cstdlib>
#include <mutex>

#include "session.h"

// ---------------------------------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------------------------------
thread_local std::string g_err;
int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// ---------------------------------------------------------------------------------------------------------------------
// tuning switches: one table, read from the environment once (kernels.h: EmmaxTune)
// ---------------------------------------------------------------------------------------------------------------------
namespace {
struct TuneEntry { const char* name; int EmmaxTune::*field; int def; };
const TuneEntry kTune[] = {
    {"graph", &EmmaxTune::graph, 0},           {"ks", &EmmaxTune::ks, 1},
    {"ks_oproj", &EmmaxTune::ks_oproj, 1},     {"ks_oproj_grid", &EmmaxTune::ks_oproj_grid, 256},
    {"km", &EmmaxTune::km, 1},                 {"km_down", &EmmaxTune::km_down, 1},
    {"km_roll", &EmmaxTune::km_roll, 0},       {"attn_nw", &EmmaxTune::attn_nw, 4},
    {"attn_deep", &EmmaxTune::attn_deep, -1},  {"attn_ksplit", &EmmaxTune::attn_ksplit, -1},
    {"attn_lazy", &EmmaxTune::attn_lazy, 1},      {"vis_streams", &EmmaxTune::vis_streams, 1},
    {"streamk", &EmmaxTune::streamk, 1},       {"fp8_gemv", &EmmaxTune::fp8_gemv, -1},
    {"attn_nsplit", &EmmaxTune::attn_nsplit, 0}, {"attn_direct", &EmmaxTune::attn_direct, 1},
    {"fold_embed", &EmmaxTune::fold_embed, 1}, {"mfma_xbar", &EmmaxTune::mfma_xbar, 1},
    {"gemm_big", &EmmaxTune::gemm_big, -1},    {"gemm_splitk", &EmmaxTune::gemm_splitk, 1},
    {"gemm_sk_big", &EmmaxTune::gemm_sk_big, -1},
    {"gemm_deep", &EmmaxTune::gemm_deep, -1},       {"gemm_dbg", &EmmaxTune::gemm_dbg, 0},
    {"gemm_lnfuse", &EmmaxTune::gemm_lnfuse, 1}, {"attn_resident", &EmmaxTune::attn_resident, -1},
    {"gemm_hybrid", &EmmaxTune::gemm_hybrid, 1}, {"gemm_normfuse", &EmmaxTune::gemm_normfuse, 1},
    {"resid32", &EmmaxTune::resid32, 1},       {"kv_fp8", &EmmaxTune::kv_fp8, 0},
    {"exact", &EmmaxTune::exact, 0},           {"attn_group", &EmmaxTune::attn_group, -1},
    {"mx4_wide", &EmmaxTune::mx4_wide, 0},
};
EmmaxTune g_tune;
std::once_flag g_tune_once;
void tune_init() {
    g_tune.epoch = 0;
    for (const TuneEntry& e : kTune) {
        g_tune.*(e.field) = e.def;
        std::string env = "EMMAX_";
        for (const char* c = e.name; *c; ++c) env += (char)toupper((unsigned char)*c);
        if (const char* v = getenv(env.c_str())) g_tune.*(e.field) = atoi(v);   // the ONLY getenv of the library
    }
}
}  // namespace
const EmmaxTune& emmax_tune() {
    std::call_once(g_tune_once, tune_init);
    return g_tune;
}

// hipGraph replay of the decode step (tuning switch graph): ROCm 7.2's default replay path ("graph packet capture") adds ~0.65 us per kernel
// node on the device (2.69 against 2.57 ms/token at B = 1); with DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 the replay runs at the rate of eager launches
// (profiles/r05_graph_switches.txt).  The HIP runtime reads the variable ONCE, at its first call -- so it is exported when THIS LIBRARY IS
// LOADED (a constructor; never overriding a value the host set), which makes the replay fast however graph mode is switched on later
// (EMMAX_GRAPH=1 or emmax_tuning_set("graph", 1)), provided the host loads libemmax_hip.so before its first HIP call -- the Python package
// does (emmax/__init__.py sets the same variable at import).  VERDICT r05 next #6.
__attribute__((constructor)) static void emmax_export_runtime_switches() { setenv("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0", 0); }

// format_rules = false: everything but the MXFP4 shape rules (emmax_config_max_decode_batch asks the planner instead)
static int check_config(const emmax_config& c, bool format_rules = true) {
    for (int t = 0; t < 2; ++t) {
        const auto& w = c.tower[t];
        if (w.embed_dim <= 0 || w.num_heads <= 0 || w.embed_dim % w.num_heads) return fail(EMMAX_ERR_INVALID, "tower %d: bad embed_dim/num_heads", t);
        const int hd = w.embed_dim / w.num_heads;
        if (hd != 64 && hd != 72) return fail(EMMAX_ERR_INVALID, "tower %d: head_dim %d outside the hot path (64 or 72)", t, hd);
        if (w.embed_dim % 8 || w.mlp_hidden % 8) return fail(EMMAX_ERR_INVALID, "tower %d: dims must be multiples of 8", t);
        if (w.take_index < 0 || w.take_index >= w.depth) return fail(EMMAX_ERR_INVALID, "tower %d: take_index out of range", t);
        if (w.image_size % w.patch) return fail(EMMAX_ERR_INVALID, "tower %d: image_size %% patch != 0", t);
    }
    if (c.tower[0].image_size != c.tower[1].image_size || c.tower[0].patch != c.tower[1].patch)
        return fail(EMMAX_ERR_INVALID, "towers must share image size and patch size");
    if (c.head_dim != 128) return fail(EMMAX_ERR_INVALID, "LLM head_dim %d outside the hot path (128)", c.head_dim);
    if (c.hidden % 128) return fail(EMMAX_ERR_INVALID, "LLM hidden must be a multiple of 128");
    if (c.n_heads % c.n_kv_heads) return fail(EMMAX_ERR_INVALID, "n_heads %% n_kv_heads != 0");
    const int G = c.n_heads / c.n_kv_heads;
    if (G != 1 && G != 2 && G != 4 && G != 8) return fail(EMMAX_ERR_INVALID, "GQA group %d unsupported (1,2,4,8)", G);
    if (c.inter % 16) return fail(EMMAX_ERR_INVALID, "LLM intermediate size must be a multiple of 16");
    if (c.vocab % 8) return fail(EMMAX_ERR_INVALID, "vocab must be a multiple of 8");
    const int wfmt = wfmt_of_code(c.decode_fp8);
    if (wfmt < 0) return fail(EMMAX_ERR_INVALID, "decode_fp8 %d: 0 (bf16), 1 (fp8-e4m3), 2 (MXFP4) or 4 (MXFP6)", c.decode_fp8);
    if (wfmt == PW_FP8 && (c.hidden % 64 || (c.n_heads * c.head_dim) % 64)) return fail(EMMAX_ERR_INVALID, "fp8 decode needs K % 64 == 0");
    if (wfmt_is_mx(wfmt) && format_rules) {
        const char* const fmt = WFMT[wfmt].name;   // (MXFP6 tiles cover the same 16 rows x 128 k per load step: one set of rules)
        // MXFP4 tiles are read by decode_km.hip alone, at every batch: the model must be a shape that file takes.  qkv / o-proj / gate-up / lm-head:
        // eight waves x whole load steps of 128 elements, at most sixteen fragments per wave -- K % 1024 == 0 and K <= 4096, at most 8 tiles
        // for each of 256 blocks (N <= 32768); the down projection on the phased kernel: whole load steps (K % 128 == 0), K above 4096 and
        // within the phases (two of six steps at 1-8 rows, four of three at 9-16: ceil(K / 128 / 8) <= 12, K <= 12288).  This runs before a model
        // exists, so it is text; emmax_config_max_decode_batch asks the planner about the same config, and tests/test_decode_plan.py holds the
        // two together (accepted exactly when the planner serves 8 rows)
        const int q_dim = c.n_heads * c.head_dim, qkv_dim = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim;
        if (c.hidden % 1024 || c.hidden > 4096 || q_dim % 1024 || q_dim > 4096)
            return fail(EMMAX_ERR_INVALID, "%s decode weights need hidden (%d) and n_heads * head_dim (%d) in multiples of 1024 up to 4096", fmt, c.hidden, q_dim);
        if (c.inter % 128 || c.inter <= 4096 || c.inter > 12288)
            return fail(EMMAX_ERR_INVALID, "%s decode weights need an intermediate size (%d) that is a multiple of 128, above 4096 and at most 12288", fmt, c.inter);
        if (qkv_dim > 32768 || 2 * c.inter > 32768 || pad_to(c.vocab, 128) > 32768)
            return fail(EMMAX_ERR_INVALID, "%s decode weights need at most 32768 rows per projection (qkv %d, gate/up %d, vocab %d)", fmt, qkv_dim, 2 * c.inter, c.vocab);
    }
    return 0;
}

// the four projections of a decoder layer, in the order of their stages: rows N and columns K of the matrix, the row order of decode_km.hip's
// copy (launch_repack_km's perm / head_dim; 0: natural -- that kernel reads the fragment-major copy) and how the step launches it (ProjW)
struct ProjDim { int stage; int64_t N, K; int perm, perm_hd, gemv_mode, f8bit; };
static std::array<ProjDim, 4> layer_projs(const emmax_model* m) {
    return {{{STAGE_QKV, m->qkv_dim, m->H, 1, m->cfg.head_dim, GEMV_QKV, F8_QKV}, {STAGE_OPROJ, m->H, m->q_dim, 0, 0, GEMV_RESID, F8_OPROJ},
             {STAGE_GATEUP, 2 * (int64_t)m->inter_p, m->H, 2, 0, GEMV_GATEUP, F8_GATEUP}, {STAGE_DOWN, m->H, m->inter_p, 0, 0, GEMV_RESID, F8_DOWN}}};
}

static void derive(emmax_model* m) {
    const auto& c = m->cfg;
    m->H = c.hidden;
    m->inter = c.inter;
    m->inter_p = pad_to(c.inter, 64);
    m->q_dim = c.n_heads * c.head_dim;
    m->kv_dim = c.n_kv_heads * c.head_dim;
    m->qkv_dim = m->q_dim + 2 * m->kv_dim;
    m->vocab = c.vocab;
    m->vocab_p = pad_to(c.vocab, 128);
    m->V = c.tower[0].embed_dim + c.tower[1].embed_dim;
    m->Vp = pad_to(m->V, 128);
    m->P1 = 4 * m->V;
    m->P1p = pad_to(m->P1, 128);
    for (int t = 0; t < 2; ++t) {
        const auto& w = c.tower[t];
        TowerW& T = m->tw[t];
        T.D = w.embed_dim;
        T.Dp = pad_to(T.D, 128);
        T.D3p = pad_to(3 * T.D, 128);
        T.M = w.mlp_hidden;
        T.Mp = pad_to(T.M, 128);
        T.n_prefix = (w.has_cls ? 1 : 0) + w.n_reg;
        T.n_patches = (w.image_size / w.patch) * (w.image_size / w.patch);
        T.N = T.n_prefix + T.n_patches;
        T.hd = T.D / w.num_heads;
        T.Kpe = pad_to(3 * w.patch * w.patch, 64);
        T.n_blocks = w.take_index + 1;   // blocks after take_index never influence the output
        T.blk.resize(T.n_blocks);
    }
    m->layers.resize(c.n_layers);
    for (auto& L : m->layers) {
        memset(&L, 0, sizeof(L));
        for (const ProjDim& d : layer_projs(m)) { L.proj[d.stage].gemv_mode = d.gemv_mode; L.proj[d.stage].f8bit = d.f8bit; }
    }
    m->lm_head_w = ProjW{};
    m->lm_head_w.gemv_mode = GEMV_LMHEAD; m->lm_head_w.f8bit = F8_LMHEAD;
    m->wfmt = wfmt_of_code(c.decode_fp8);   // (check_config has refused a code that is no format)
    // the tuning switch mx4_wide is read HERE, once (emmax_model_create; emmax_config_max_decode_batch's model of the moment), and frozen: planner,
    // session checks and launch_proj ask the model, never the live switch
    m->mx4_wide = m->wfmt == PW_MX4 && emmax_tune().mx4_wide != 0;   // (MXFP6: does not apply, decode_kmp.hip has no MX6 form)
    for (auto& L : m->layers)
        for (const ProjDim& d : layer_projs(m)) { L.proj[d.stage].wfmt = m->wfmt; L.proj[d.stage].wide = m->mx4_wide; }
    m->lm_head_w.wfmt = m->wfmt; m->lm_head_w.wide = m->mx4_wide;
}

static void plan_arena(emmax_model* m, Bump& b) {
    for (int t = 0; t < 2; ++t) {
        TowerW& T = m->tw[t];
        T.patch_w = b.take((int64_t)T.Dp * T.Kpe);
        T.patch_b = b.take(T.Dp);
        T.pos = b.take((int64_t)T.n_patches * T.D);
        T.cls = b.take(T.D);
        T.reg = b.take((int64_t)std::max(1, m->cfg.tower[t].n_reg) * T.D);
        for (auto& k : T.blk) {
            k.n1w = b.take(T.D); k.n1b = b.take(T.D);
            k.qkv_w = b.take((int64_t)T.D3p * T.Dp); k.qkv_b = b.take(T.D3p);
            k.proj_w = b.take((int64_t)T.Dp * T.Dp); k.proj_b = b.take(T.Dp);
            k.ls1 = b.take(T.Dp);
            k.n2w = b.take(T.D); k.n2b = b.take(T.D);
            k.fc1_w = b.take((int64_t)T.Mp * T.Dp); k.fc1_b = b.take(T.Mp);
            k.fc2_w = b.take((int64_t)T.Dp * T.Mp); k.fc2_b = b.take(T.Dp);
            k.ls2 = b.take(T.Dp);
            k.ln1_s = (float*)b.take(2 * (int64_t)T.D3p); k.ln1_c = (float*)b.take(2 * (int64_t)T.D3p);
            k.ln2_s = (float*)b.take(2 * (int64_t)T.Mp); k.ln2_c = (float*)b.take(2 * (int64_t)T.Mp);
        }
    }
    m->pj1_w = b.take((int64_t)m->P1p * m->Vp); m->pj1_b = b.take(m->P1p);
    m->pj2_w = b.take((int64_t)m->H * m->P1p); m->pj2_b = b.take(m->H);
    m->pj3_w = b.take((int64_t)m->H * m->H); m->pj3_b = b.take(m->H);
    m->embed = b.take((int64_t)m->vocab * m->H);
    for (auto& L : m->layers) {
        const auto dims = layer_projs(m);   // [0..3]: qkv, o-proj, gate-up, down
        ProjW *const q = &L.proj[STAGE_QKV], *const o = &L.proj[STAGE_OPROJ], *const g = &L.proj[STAGE_GATEUP], *const d = &L.proj[STAGE_DOWN];
        L.ln1 = b.take(m->H);
        q->rm = b.take(dims[0].N * dims[0].K);
        o->rm = b.take(dims[1].N * dims[1].K);
        L.ln2 = b.take(m->H);
        g->rm = b.take(dims[2].N * dims[2].K);
        d->rm = b.take(dims[3].N * dims[3].K);
        for (const ProjDim& p : dims) { ProjW& w = L.proj[p.stage]; w.r8 = nullptr; w.sc = w.km_sc = nullptr; w.tiles = w.codes = nullptr; }
        if (m->is_mx())   // 4.25 / 6.25 bits per weight: every batch reads these, so they live in the main arena
            for (const ProjDim& p : dims) { ProjW& w = L.proj[p.stage]; w.tiles = b.bytes(wfmt_bytes(m->wfmt, p.N, p.K)); w.codes = b.bytes(wfmt_scale_bytes(m->wfmt, p.N, p.K)); }
        if (m->wfmt == PW_FP8) {   // fp8 tiles take half the bytes; every batch regime reads some of them, so they live in the main arena
            for (const ProjDim& p : dims) L.proj[p.stage].fm = b.take(p.N * p.K / 2);
            q->km = b.take(dims[0].N * dims[0].K / 2);
            g->km = b.take(dims[2].N * dims[2].K / 2);
            for (const ProjDim& p : dims) L.proj[p.stage].r8 = b.take(p.N * p.K / 2);
            for (const ProjDim& p : dims) L.proj[p.stage].sc = (float*)b.take(2 * p.N);
            q->km_sc = (float*)b.take(2 * dims[0].N);
            g->km_sc = (float*)b.take(2 * dims[2].N);
            o->km = o->fm; o->km_sc = o->sc;
            d->km = d->fm; d->km_sc = d->sc;
        }
    }
    m->final_norm = b.take(m->H);
    ProjW& lm = m->lm_head_w;
    lm.rm = b.take((int64_t)m->vocab_p * m->H);
    if (m->wfmt == PW_FP8) {
        lm.km = lm.fm = b.take((int64_t)m->vocab_p * m->H / 2);
        lm.km_sc = lm.sc = (float*)b.take(2 * (int64_t)m->vocab_p);
        lm.r8 = b.take((int64_t)m->vocab_p * m->H / 2);
    }
    if (m->is_mx()) { lm.tiles = b.bytes(wfmt_bytes(m->wfmt, m->vocab_p, m->H)); lm.codes = b.bytes(wfmt_scale_bytes(m->wfmt, m->vocab_p, m->H)); }
}

// bf16 models: the copies only the batch >= 3 decode kernels read -- row-permuted fragment-major qkv / gate-up (decode_km.hip),
// fragment-major o-proj / down / lm-head (decode_km.hip's natural-order form and decode_mfma.hip) -- live in a SECOND arena that
// a model serving batches 1-2 never needs (13.2 GB at 7B).  The fragment-major qkv / gate-up pair of decode_mfma.hip is the A/B
// partner of decode_km.hip and is built only when the tuning switch km is 0 at build time (+9 GB).
static void plan_aux(emmax_model* m, Bump& b, bool with_ab_partner) {
    for (auto& L : m->layers) {
        const auto dims = layer_projs(m);   // [0..3]: qkv, o-proj, gate-up, down
        ProjW *const q = &L.proj[STAGE_QKV], *const o = &L.proj[STAGE_OPROJ], *const g = &L.proj[STAGE_GATEUP], *const d = &L.proj[STAGE_DOWN];
        q->km = b.take(dims[0].N * dims[0].K);
        g->km = b.take(dims[2].N * dims[2].K);
        o->km = o->fm = b.take(dims[1].N * dims[1].K);
        d->km = d->fm = b.take(dims[3].N * dims[3].K);
        q->fm = with_ab_partner ? b.take(dims[0].N * dims[0].K) : nullptr;
        g->fm = with_ab_partner ? b.take(dims[2].N * dims[2].K) : nullptr;
    }
    m->lm_head_w.km = m->lm_head_w.fm = b.take((int64_t)m->vocab_p * m->H);
}

// copy a bound [rows, cols] bf16 matrix into dst (row pitch dst_ld elements) starting at dst row `row0`
static int put2d(emmax_model* m, const std::string& key, int rows, int cols, bf16* dst, int dst_ld, int row0, hipStream_t st) {
    auto it = m->bound.find(key);
    if (it == m->bound.end()) return fail(EMMAX_ERR_MISSING, "finalize: weight `%s` was never bound", key.c_str());
    const Bound& w = it->second;
    if (w.dtype != EMMAX_BF16) return fail(EMMAX_ERR_INVALID, "weight `%s` must be bf16", key.c_str());
    if (w.numel() != (int64_t)rows * cols)
        return fail(EMMAX_ERR_INVALID, "weight `%s`: expected %d x %d = %lld elements, got %lld", key.c_str(), rows, cols,
                    (long long)rows * cols, (long long)w.numel());
    HIPCHK(hipMemcpy2DAsync(dst + (size_t)row0 * dst_ld, (size_t)dst_ld * 2, w.ptr, (size_t)cols * 2, (size_t)cols * 2, rows,
                            hipMemcpyDeviceToDevice, st));
    return 0;
}
static int put1d(emmax_model* m, const std::string& key, int n, bf16* dst, hipStream_t st) { return put2d(m, key, 1, n, dst, n, 0, st); }

// ---------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------
extern "C" {

const char* emmax_version(void) { return "emmax-hip 0.1.0 (gfx950)"; }
const char* emmax_last_error(void) { return g_err.c_str(); }
int emmax_abi_version(void) { return EMMAX_ABI_VERSION; }
int emmax_config_size(void) { return (int)sizeof(emmax_config); }

int emmax_tuning_set(const char* name, int value) {
    if (!name) return fail(EMMAX_ERR_INVALID, "null argument");
    (void)emmax_tune();
    for (const TuneEntry& e : kTune)
        if (!strcmp(e.name, name)) {
            g_tune.*(e.field) = value;
            g_tune.epoch += 1;
            return 0;
        }
    return fail(EMMAX_ERR_INVALID, "unknown tuning switch `%s`", name);
}
int emmax_tuning_get(const char* name, int* value_out) {
    if (!name || !value_out) return fail(EMMAX_ERR_INVALID, "null argument");
    const EmmaxTune& t = emmax_tune();
    for (const TuneEntry& e : kTune)
        if (!strcmp(e.name, name)) {
            *value_out = t.*(e.field);
            return 0;
        }
    return fail(EMMAX_ERR_INVALID, "unknown tuning switch `%s`", name);
}

int emmax_model_create(const emmax_config* cfg, emmax_model** out) {
    if (!cfg || !out) return fail(EMMAX_ERR_INVALID, "null argument");
    int r = check_config(*cfg);
    if (r) return r;
    emmax_model* m = new emmax_model();
    m->cfg = *cfg;
    derive(m);
    *out = m;
    return 0;
}

void emmax_model_destroy(emmax_model* m) { delete m; }

int emmax_model_bind_weight(emmax_model* m, const char* key, const void* ptr, int dtype, const int64_t* shape, int ndim) {
    if (!m || !key || !ptr || (ndim > 0 && !shape)) return fail(EMMAX_ERR_INVALID, "null argument");
    if (m->finalized) return fail(EMMAX_ERR_STATE, "model already finalized");
    Bound b;
    b.ptr = ptr; b.dtype = dtype;
    b.shape.assign(shape, shape + ndim);
    m->bound[key] = b;
    return 0;
}

int64_t emmax_model_arena_bytes(const emmax_model* m) {
    if (!m) return -1;
    Bump b{nullptr};
    plan_arena(const_cast<emmax_model*>(m), b);
    return b.off + 256;
}

int emmax_model_finalize(emmax_model* m, void* arena, int64_t arena_bytes, emmax_stream stream) {
    if (!m || !arena) return fail(EMMAX_ERR_INVALID, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const int64_t need = emmax_model_arena_bytes(m);
    if (arena_bytes < need) return fail(EMMAX_ERR_NOMEM, "arena too small: %lld < %lld", (long long)arena_bytes, (long long)need);
    if ((uintptr_t)arena % 256) return fail(EMMAX_ERR_INVALID, "arena must be 256-byte aligned");
    Bump b{(char*)arena};
    plan_arena(m, b);
    HIPCHK(hipMemsetAsync(arena, 0, need, st));   // all padding is zero
    const char* pre[2] = {"vision_backbone.featurizer.", "vision_backbone.fused_featurizer."};
    const bool fold_ln = emmax_tune().gemm_lnfuse != 0 && emmax_tune().exact == 0;   // exact numerics multiplies by the checkpoint's weights, not by bf16(W .* gamma)
    int r;
#define PUT2(key, rows, cols, dst, ld, row0) if ((r = put2d(m, key, rows, cols, dst, ld, row0, st))) return r
#define PUT1(key, n, dst) if ((r = put1d(m, key, n, dst, st))) return r
    for (int t = 0; t < 2; ++t) {
        TowerW& T = m->tw[t];
        const emmax_tower_config& tc = m->cfg.tower[t];
        const std::string P = pre[t];
        PUT2(P + "patch_embed.proj.weight", T.D, 3 * tc.patch * tc.patch, T.patch_w, T.Kpe, 0);
        PUT1(P + "patch_embed.proj.bias", T.D, T.patch_b);
        PUT1(P + "pos_embed", T.n_patches * T.D, T.pos);
        if (tc.has_cls) PUT1(P + "cls_token", T.D, T.cls);
        if (tc.n_reg) PUT1(P + "reg_token", tc.n_reg * T.D, T.reg);
        for (int i = 0; i < T.n_blocks; ++i) {
            BlockW& k = T.blk[i];
            const std::string Bp = P + "blocks." + std::to_string(i) + ".";
            PUT1(Bp + "norm1.weight", T.D, k.n1w); PUT1(Bp + "norm1.bias", T.D, k.n1b);
            PUT2(Bp + "attn.qkv.weight", 3 * T.D, T.D, k.qkv_w, T.Dp, 0); PUT1(Bp + "attn.qkv.bias", 3 * T.D, k.qkv_b);
            PUT2(Bp + "attn.proj.weight", T.D, T.D, k.proj_w, T.Dp, 0); PUT1(Bp + "attn.proj.bias", T.D, k.proj_b);
            PUT1(Bp + "norm2.weight", T.D, k.n2w); PUT1(Bp + "norm2.bias", T.D, k.n2b);
            PUT2(Bp + "mlp.fc1.weight", T.M, T.D, k.fc1_w, T.Dp, 0); PUT1(Bp + "mlp.fc1.bias", T.M, k.fc1_b);
            PUT2(Bp + "mlp.fc2.weight", T.D, T.M, k.fc2_w, T.Mp, 0); PUT1(Bp + "mlp.fc2.bias", T.D, k.fc2_b);
            if (tc.layerscale) { PUT1(Bp + "ls1.scale_factor", T.D, k.ls1); PUT1(Bp + "ls2.scale_factor", T.D, k.ls2); }
            if (fold_ln) {   // W <- bf16(W .* gamma) in place; the norm weights stay in the arena for the un-fused A/B path of OTHER models only
                KCHK(launch_ln_fold(k.qkv_w, T.Dp, 3 * T.D, T.D, k.n1w, k.n1b, k.qkv_b, k.ln1_s, k.ln1_c, st));
                KCHK(launch_ln_fold(k.fc1_w, T.Dp, T.M, T.D, k.n2w, k.n2b, k.fc1_b, k.ln2_s, k.ln2_c, st));
            }
        }
    }
    PUT2("projector.fc1.weight", m->P1, m->V, m->pj1_w, m->Vp, 0); PUT1("projector.fc1.bias", m->P1, m->pj1_b);
    PUT2("projector.fc2.weight", m->H, m->P1, m->pj2_w, m->P1p, 0); PUT1("projector.fc2.bias", m->H, m->pj2_b);
    PUT2("projector.fc3.weight", m->H, m->H, m->pj3_w, m->H, 0); PUT1("projector.fc3.bias", m->H, m->pj3_b);
    PUT2("language_model.model.embed_tokens.weight", m->vocab, m->H, m->embed, m->H, 0);
    for (int li = 0; li < m->cfg.n_layers; ++li) {
        LayerW& L = m->layers[li];
        const std::string P = "language_model.model.layers." + std::to_string(li) + ".";
        PUT1(P + "input_layernorm.weight", m->H, L.ln1);
        PUT2(P + "self_attn.q_proj.weight", m->q_dim, m->H, L.proj[STAGE_QKV].rm, m->H, 0);
        PUT2(P + "self_attn.k_proj.weight", m->kv_dim, m->H, L.proj[STAGE_QKV].rm, m->H, m->q_dim);
        PUT2(P + "self_attn.v_proj.weight", m->kv_dim, m->H, L.proj[STAGE_QKV].rm, m->H, m->q_dim + m->kv_dim);
        PUT2(P + "self_attn.o_proj.weight", m->H, m->q_dim, L.proj[STAGE_OPROJ].rm, m->q_dim, 0);
        PUT1(P + "post_attention_layernorm.weight", m->H, L.ln2);
        // gate/up interleaved in 16-row groups: dst rows [32j, 32j+16) = gate rows [16j, 16j+16), next 16 = up
        {
            auto ig = m->bound.find(P + "mlp.gate_proj.weight");
            auto iu = m->bound.find(P + "mlp.up_proj.weight");
            if (ig == m->bound.end() || iu == m->bound.end()) return fail(EMMAX_ERR_MISSING, "finalize: gate/up of layer %d not bound", li);
            if (ig->second.numel() != (int64_t)m->inter * m->H || iu->second.numel() != (int64_t)m->inter * m->H)
                return fail(EMMAX_ERR_INVALID, "gate/up of layer %d have the wrong size", li);
            const size_t grp = (size_t)16 * m->H * 2;
            HIPCHK(hipMemcpy2DAsync(L.proj[STAGE_GATEUP].rm, 2 * grp, ig->second.ptr, grp, grp, m->inter / 16, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpy2DAsync((char*)L.proj[STAGE_GATEUP].rm + grp, 2 * grp, iu->second.ptr, grp, grp, m->inter / 16, hipMemcpyDeviceToDevice, st));
        }
        PUT2(P + "mlp.down_proj.weight", m->H, m->inter, L.proj[STAGE_DOWN].rm, m->inter_p, 0);
        if (m->wfmt == PW_FP8) {
            const auto dims = layer_projs(m);
            for (const ProjDim& d : dims) KCHK(launch_quant_fm8(L.proj[d.stage].rm, (int)d.K, L.proj[d.stage].fm, L.proj[d.stage].sc, (int)d.N, (int)d.K, st));
            for (const ProjDim& d : dims)   // (writes the same scales again)
                KCHK(launch_quant_rm8(L.proj[d.stage].rm, (int)d.K, L.proj[d.stage].r8, L.proj[d.stage].sc, (int)d.N, (int)d.K, st));
            for (const ProjDim& d : dims)
                if (d.perm) KCHK(launch_quant_fm8(L.proj[d.stage].rm, (int)d.K, L.proj[d.stage].km, L.proj[d.stage].km_sc, (int)d.N, (int)d.K, st, d.perm, d.perm_hd));
        }
        if (m->is_mx())   // quantise, then write the values the copy holds back over the rows the prefill GEMMs read (exact in bf16): prefill, extend,
                          // verify, scoring and the taps evaluate the quantised model
            for (const ProjDim& d : layer_projs(m)) {
                ProjW& w = L.proj[d.stage];
                KCHK(launch_quant_mx(m->wfmt, w.rm, (int)d.K, w.tiles, w.codes, (int)d.N, (int)d.K, d.perm, d.perm_hd, st));
                KCHK(launch_dequant_mx(m->wfmt, w.tiles, w.codes, w.rm, (int)d.K, (int)d.N, (int)d.K, d.perm, d.perm_hd, st));
            }
    }
    PUT1("language_model.model.norm.weight", m->H, m->final_norm);
    PUT2("language_model.lm_head.weight", m->vocab, m->H, m->lm_head_w.rm, m->H, 0);
    if (m->wfmt == PW_FP8) {
        KCHK(launch_quant_fm8(m->lm_head_w.rm, m->H, m->lm_head_w.fm, m->lm_head_w.sc, m->vocab_p, m->H, st));
        KCHK(launch_quant_rm8(m->lm_head_w.rm, m->H, m->lm_head_w.r8, m->lm_head_w.sc, m->vocab_p, m->H, st));
    }
    if (m->is_mx()) {
        KCHK(launch_quant_mx(m->wfmt, m->lm_head_w.rm, m->H, m->lm_head_w.tiles, m->lm_head_w.codes, m->vocab_p, m->H, 0, 0, st));
        KCHK(launch_dequant_mx(m->wfmt, m->lm_head_w.tiles, m->lm_head_w.codes, m->lm_head_w.rm, m->H, m->vocab_p, m->H, 0, 0, st));
    }
#undef PUT2
#undef PUT1
    HIPCHK(hipStreamSynchronize(st));
    m->finalized = true;
    m->ln_folded = fold_ln;
    m->aux_built = m->wfmt != PW_BF16;
    m->bound.clear();
    return 0;
}

int emmax_model_max_decode_batch(const emmax_model* m) { return m ? model_max_decode_batch(m) : -1; }
int emmax_model_max_decode_batch_exact(const emmax_model* m) { return m ? model_max_decode_batch(m, true) : -1; }
int emmax_model_mxfp4_wide(const emmax_model* m) { return m ? (m->mx4_wide ? 1 : 0) : -1; }
int emmax_config_max_decode_batch(const emmax_config* cfg, int exact) {
    if (!cfg) return fail(EMMAX_ERR_INVALID, "null argument");
    if (int r = check_config(*cfg, false)) return r;
    emmax_model tmp;
    tmp.cfg = *cfg;
    derive(&tmp);
    return model_max_decode_batch(&tmp, exact != 0);
}

int64_t emmax_model_aux_bytes(const emmax_model* m) {
    if (!m) return -1;
    if (m->wfmt != PW_BF16) return 0;
    // sized on a copy of the layer table: a const query must not move the pointers of a built arena
    emmax_model tmp = *m;
    Bump b{nullptr};
    plan_aux(&tmp, b, emmax_tune().km == 0);
    return b.off + 256;
}

int emmax_model_build_aux(emmax_model* m, void* aux, int64_t aux_bytes, emmax_stream stream) {
    if (!m) return fail(EMMAX_ERR_INVALID, "null argument");
    if (!m->finalized) return fail(EMMAX_ERR_STATE, "emmax_model_build_aux before emmax_model_finalize");
    if (m->wfmt != PW_BF16) return 0;   // nothing to build: the e4m3 / MXFP4 / MXFP6 copies of every regime are in the main arena
    if (!aux) return fail(EMMAX_ERR_INVALID, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const bool ab = emmax_tune().km == 0;
    const int64_t need = emmax_model_aux_bytes(m);
    if (aux_bytes < need) return fail(EMMAX_ERR_NOMEM, "aux arena too small: %lld < %lld", (long long)aux_bytes, (long long)need);
    if ((uintptr_t)aux % 256) return fail(EMMAX_ERR_INVALID, "aux arena must be 256-byte aligned");
    Bump b{(char*)aux};
    plan_aux(m, b, ab);
    for (auto& L : m->layers) {
        const auto dims = layer_projs(m);
        for (const ProjDim& d : dims)
            if (d.perm) KCHK(launch_repack_km(L.proj[d.stage].rm, (int)d.K, L.proj[d.stage].km, (int)d.N, (int)d.K, d.perm, d.perm_hd, st));
        for (const ProjDim& d : dims)
            if (!d.perm) KCHK(launch_repack_fm(L.proj[d.stage].rm, (int)d.K, L.proj[d.stage].fm, (int)d.N, (int)d.K, st));
        for (const ProjDim& d : dims)
            if (d.perm && ab) KCHK(launch_repack_fm(L.proj[d.stage].rm, (int)d.K, L.proj[d.stage].fm, (int)d.N, (int)d.K, st));
    }
    KCHK(launch_repack_fm(m->lm_head_w.rm, m->H, m->lm_head_w.fm, m->vocab_p, m->H, st));
    HIPCHK(hipStreamSynchronize(st));
    m->aux_built = true;
    m->aux_ab = ab;
    return 0;
}

}  // extern "C"
