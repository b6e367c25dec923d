// Host side of the C ABI: context, parameter table, workspace, dispatch.
#include "wn_common.h"
#include "wn_temper.h"
#include <ctype.h>
#include <dlfcn.h>
#include <math.h>
#include <algorithm>

std::string g_create_err;

// The one place where the library takes memory from and returns it to the runtime (wn_dev.h: every DevBuf / PinBuf goes through this pair).
hipError_t wn_dev_alloc(void** p, size_t bytes, bool pinned) {
    const hipError_t e = pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes);
    if (e != hipSuccess) *p = nullptr;
    if (*p) { ++wn_dev_counts().bufs; ++wn_dev_counts().allocs; }      // (a 0-byte request may succeed with a null pointer: nothing to own, nothing counted)
    return e;
}
void wn_dev_free(void* p, bool pinned) { (void)(pinned ? hipHostFree(p) : hipFree(p)); --wn_dev_counts().bufs; }
// test hook: live device buffers, streams, events, graph execs of this process, and buffer allocations ever
extern "C" int wn_test_device_resources(int64_t out[5]) {
    if (!out) return WN_E_ARG;
    const WnDevCounts& n = wn_dev_counts();
    out[0] = n.bufs; out[1] = n.streams; out[2] = n.events; out[3] = n.gexecs; out[4] = n.allocs;
    return WN_OK;
}

static int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

static void add_tensor(wn_ctx* c, const std::string& name, std::initializer_list<int> shape, int64_t* off_out) {
    WnTensor t; t.name = name; t.ndim = (int)shape.size(); t.numel = 1;
    int i = 0; for (int s : shape) { t.shape[i++] = s; t.numel *= s; }
    for (; i < 4; ++i) t.shape[i] = 1;
    t.offset = c->n_params;
    c->n_params = align_up(c->n_params + t.numel, 8);       // 32-B aligned tensors
    *off_out = t.offset;
    c->tensors.push_back(t);
}

// Flat parameter table.  Names mirror the reference's variable scopes (wavenet.py:103-205,
// modules.py:407-450); layouts are TensorFlow's.  Within a layer the cin kernel directly follows the
// dilated kernel so that d[W_dil; W_cin] is one contiguous [(3R+C), G] matrix for the wgrad kernel.
static void build_layout(wn_ctx* c) {
    char buf[160];
    add_tensor(c, "input_convolution/kernel", {1, c->Cin, c->R}, &c->first.dil_k);
    add_tensor(c, "input_convolution/bias", {c->R}, &c->first.dil_b);
    c->lay.resize(c->L);
    for (int l = 0; l < c->L; ++l) {
        WnLayerOffsets& o = c->lay[l];
        auto nm = [&](const char* s) { snprintf(buf, sizeof buf, "ResidualConv1DGLU_%d/%s", l, s); return std::string(buf); };
        add_tensor(c, nm("residual_block_causal_conv/kernel"), {3, c->R, c->G}, &o.dil_k);
        add_tensor(c, nm("residual_block_cin_conv/kernel"), {1, c->C, c->G}, &o.cin_k);
        o.dil_b = o.cin_b = o.skip_b = o.out_b = -1;
        if (c->lbias) {          // use_bias (hparams.py:189) governs only the convolutions inside ResidualConv1DGLU (modules.py:399-446)
            add_tensor(c, nm("residual_block_causal_conv/bias"), {c->G}, &o.dil_b);
            add_tensor(c, nm("residual_block_cin_conv/bias"), {c->G}, &o.cin_b);
        }
        if (c->gin > 0) {
            add_tensor(c, nm("residual_block_gin_conv/kernel"), {1, c->gin, c->G}, &o.gin_k);
            if (c->lbias) add_tensor(c, nm("residual_block_gin_conv/bias"), {c->G}, &o.gin_b);
        }
        add_tensor(c, nm("residual_block_skip_conv/kernel"), {1, c->GH, c->S}, &o.skip_k);
        add_tensor(c, nm("residual_block_out_conv/kernel"), {1, c->GH, c->R}, &o.out_k);
        if (c->lbias) {
            add_tensor(c, nm("residual_block_skip_conv/bias"), {c->S}, &o.skip_b);
            add_tensor(c, nm("residual_block_out_conv/bias"), {c->R}, &o.out_b);
        }
    }
    add_tensor(c, "final_convolution_1/kernel", {1, c->S, c->S}, &c->fin1_k);
    add_tensor(c, "final_convolution_1/bias", {c->S}, &c->fin1_b);
    add_tensor(c, "final_convolution_2/kernel", {1, c->S, c->O}, &c->fin2_k);
    add_tensor(c, "final_convolution_2/bias", {c->O}, &c->fin2_b);
    const wn_config& g = c->cfg;
    if (c->gin > 0 && g.use_speaker_embedding) add_tensor(c, "gc_embedding", {g.n_speakers, c->gin}, &c->emb_off);   // modules.py:13-17
    if (g.upsample_type != WN_UP_NEAREST) {
        for (int i = 0; i < g.n_upsample; ++i) {
            int s = g.upsample_scales[i], fk = g.freq_axis_kernel_size;
            int64_t ko, bo;
            snprintf(buf, sizeof buf, "local_conditioning_upsampling_%d/kernel", i + 1);
            std::string kn = buf;
            snprintf(buf, sizeof buf, "local_conditioning_upsampling_%d/bias", i + 1);
            std::string bn = buf;
            if (g.upsample_type == WN_UP_2D) { add_tensor(c, kn, {fk, s, 1, 1}, &ko); add_tensor(c, bn, {1}, &bo); }
            else if (g.upsample_type == WN_UP_SUBPIXEL) { add_tensor(c, kn, {fk, 3, 1, s}, &ko); add_tensor(c, bn, {s}, &bo); }
            else if (g.upsample_type == WN_UP_RESIZE) { add_tensor(c, kn, {fk, s, 1, 1}, &ko); add_tensor(c, bn, {1}, &bo); }
            else { add_tensor(c, kn, {1, s, c->C, c->C}, &ko); add_tensor(c, bn, {c->C}, &bo); }
            c->up_k.push_back(ko); c->up_b.push_back(bo);
        }
    }
    // ---- exported (raw) layout.  With weight normalisation every convolution kernel gets a gain vector g over its LAST axis
    // (WeightNorm.build: layer_depth = kernel.shape[-1], modules.py:152-166) right behind it; biases / embedding unchanged.
    c->n_raw = 0;
    for (const WnTensor& t : c->tensors) {
        const bool is_kernel = c->wnorm && t.name.size() > 7 && t.name.compare(t.name.size() - 7, 7, "/kernel") == 0;
        WnTensor r = t; r.offset = c->n_raw; c->n_raw = align_up(c->n_raw + r.numel, 8);
        c->raw_tensors.push_back(r);
        wn_ctx::WnMap m; m.raw_off = r.offset; m.eff_off = t.offset; m.numel = t.numel; m.g_off = -1; m.cout = t.shape[t.ndim - 1]; m.pad = 0;
        if (is_kernel) {
            WnTensor g; g.name = t.name.substr(0, t.name.size() - 6) + "g"; g.ndim = 1; g.shape[0] = m.cout; g.shape[1] = g.shape[2] = g.shape[3] = 1;
            g.numel = m.cout; g.offset = c->n_raw; c->n_raw = align_up(c->n_raw + g.numel, 8);
            m.g_off = g.offset;
            c->raw_tensors.push_back(g);
        }
        c->wmap.push_back(m);
    }
    if (!c->lbias) {      // absent layer biases READ from the zero tail behind the ctx-owned parameter copy
        c->zpad = (int)align_up(std::max(std::max(c->G, c->S), c->R), 8);
        for (auto& o : c->lay) { o.dil_b = o.cin_b = o.skip_b = o.out_b = c->n_params; if (c->gin > 0) o.gin_b = c->n_params; }
    }
}

static char* bump(char*& p, size_t bytes) { char* r = p; p += align_up((int64_t)bytes, 256); return r; }

// Inference-only contexts (cfg.inference_only) keep what Fast-WaveNet synthesis touches: the upsampled conditioning (cbt + the
// fp32 levels of the upsample net), scalars and the zero page.  Everything else below is saved-activation / backward workspace.
static int alloc_workspace_inference(wn_ctx* c) {
    const int64_t NT = c->NT;
    size_t total = 0;
    auto sz = [&](size_t b) { total += align_up((int64_t)b, 256); };
    // level i of the upsample net holds Tc * prod(scales[0..i]) samples per stream: only the last one is full rate
    std::vector<int64_t> lvl(c->cfg.n_upsample + 1, NT);
    if (c->cfg.upsample_type != WN_UP_NEAREST) {
        int64_t den = c->hop;
        for (int i = 0; i < c->cfg.n_upsample; ++i) { den /= c->cfg.upsample_scales[i]; lvl[i] = NT / (den > 0 ? den : 1) + c->maxB; }
    }
    sz(NT * c->C * 2);
    for (int i = 0; i <= c->cfg.n_upsample; ++i) sz(lvl[i] * c->C * 4);
    sz(256); sz(WN_ZERO_PAGE_BYTES);
    sz((size_t)wn_score_part_doubles(c->maxB, c->maxT) * 8);      // wn_score partials: scoring never allocates
    WN_HIP(c, c->ws.reserve(total));
    char* p = c->ws;
    c->cbt = (bf16_t*)bump(p, NT * c->C * 2);
    for (int i = 0; i <= c->cfg.n_upsample; ++i) c->CUP[i] = (float*)bump(p, lvl[i] * c->C * 4);
    c->scal = (float*)bump(p, 256);
    c->zero_page = (bf16_t*)bump(p, WN_ZERO_PAGE_BYTES);
    c->score_part = (double*)bump(p, (size_t)wn_score_part_doubles(c->maxB, c->maxT) * 8);
    c->X = c->XD = c->TS = c->U = c->R1 = c->H2 = c->DY = c->DPRE1 = c->DSKIP = c->DZ = c->GXall = c->GX0 = c->GX1 = nullptr;
    c->YHAT = c->DC = c->DCUP[0] = c->DCUP[1] = c->CIN = c->UPPART = nullptr; c->XIN = nullptr;
    if (hipMemset(c->zero_page, 0, WN_ZERO_PAGE_BYTES) != hipSuccess) WN_FAIL(c, WN_E_HIP, "hipMemset(zero page) failed");
    return WN_OK;
}

static int alloc_workspace(wn_ctx* c) {
    if (c->inference) return alloc_workspace_inference(c);
    const int64_t NT = c->NT;
    const int ldDY = (int)align_up(c->O, 16);
    size_t total = 0;
    auto sz = [&](size_t b) { total += align_up((int64_t)b, 256); };
    const int L = c->L;
    sz(NT * c->C * 2);                     // cbt
    sz((size_t)(L) * NT * c->R * 2);       // X[0..L-1]
    if (c->cfg.dropout > 0.0f) sz((size_t)(L) * NT * c->R * 2);   // XD
    sz((size_t)L * NT * c->GH * 2);        // TS: sigmoid half of the gate (tanh is recovered from u in the backward)
    sz((size_t)L * NT * c->GH * 2);        // U
    sz(NT * c->S * 2); sz(NT * c->S * 2);  // R1, H2
    sz(NT * ldDY * 2);                     // DY
    sz(NT * c->S * 2); sz(NT * c->S * 2);  // DPRE1, DSKIP
    sz((size_t)L * NT * c->G * 2);         // DZ
    sz((size_t)(L + 1) * NT * c->R * 2);   // GXall
    sz(NT * c->O * 4);                     // YHAT
    sz(NT * c->C * 4);                     // DC
    for (int i = 0; i <= c->cfg.n_upsample; ++i) sz(NT * c->C * 4);   // CUP (generous: every level sized for full rate)
    sz(NT * c->C * 4); sz(NT * c->C * 4);  // DCUP ping-pong
    {   // per-workgroup partial sums of the upsample-kernel gradients (wn_up_bwd_params2): (rows + 2048 slices) x (taps + biases)
        int ne = 1;
        const int fk = c->cfg.freq_axis_kernel_size;
        for (int i = 0; i < c->cfg.n_upsample; ++i) { const int s_ = c->cfg.upsample_scales[i]; ne = std::max(ne, c->cfg.upsample_type == WN_UP_2D ? fk * s_ + 1 : fk * 3 * s_ + s_); }
        c->uppart_floats = ((int64_t)c->maxB * c->C + 2048) * ne;
        sz((size_t)c->uppart_floats * 4);
    }
    sz(NT * 4); sz(NT * c->C * 4);          // XIN, CIN
    sz((size_t)WN_CS_SLOTS * WN_CS_MAXBLK * 2 * 1024 * 4);    // wn_colsum2 partials (WN_CS_SLOTS regions)
    sz(256);                               // scalars
    sz(WN_ZERO_PAGE_BYTES);                // zero page
    sz((size_t)wn_score_part_doubles(c->maxB, c->maxT) * 8);      // wn_score / wn_eval_fwd partials
    WN_HIP(c, c->ws.reserve(total));
    char* p = c->ws;
    c->cbt = (bf16_t*)bump(p, NT * c->C * 2);
    c->X = (bf16_t*)bump(p, (size_t)L * NT * c->R * 2);
    c->XD = (c->cfg.dropout > 0.0f) ? (bf16_t*)bump(p, (size_t)L * NT * c->R * 2) : c->X;
    c->TS = (bf16_t*)bump(p, (size_t)L * NT * c->GH * 2);
    c->U = (bf16_t*)bump(p, (size_t)L * NT * c->GH * 2);
    c->R1 = (bf16_t*)bump(p, NT * c->S * 2); c->H2 = (bf16_t*)bump(p, NT * c->S * 2);
    c->DY = (bf16_t*)bump(p, NT * ldDY * 2);
    c->DPRE1 = (bf16_t*)bump(p, NT * c->S * 2); c->DSKIP = (bf16_t*)bump(p, NT * c->S * 2);
    c->DZ = (bf16_t*)bump(p, (size_t)L * NT * c->G * 2);
    c->GXall = (bf16_t*)bump(p, (size_t)(L + 1) * NT * c->R * 2);
    c->GX0 = c->GXall; c->GX1 = c->GXall + (size_t)NT * c->R;     // (debug names: gradients wrt the inputs of layers 0 and 1)
    c->YHAT = (float*)bump(p, NT * c->O * 4);
    c->DC = (float*)bump(p, NT * c->C * 4);
    for (int i = 0; i <= c->cfg.n_upsample; ++i) c->CUP[i] = (float*)bump(p, NT * c->C * 4);
    c->DCUP[0] = (float*)bump(p, NT * c->C * 4); c->DCUP[1] = (float*)bump(p, NT * c->C * 4);
    c->UPPART = (float*)bump(p, (size_t)c->uppart_floats * 4);
    c->XIN = (void*)bump(p, NT * 4); c->CIN = (float*)bump(p, NT * c->C * 4);
    c->cs_part = (float*)bump(p, (size_t)WN_CS_SLOTS * WN_CS_MAXBLK * 2 * 1024 * 4);      // exactly what wn_colsum2 addresses (was twice that: ADVICE round 3)
    c->ws_step_bytes = (size_t)(p - (char*)c->ws);      // everything carved so far is written by training steps only (wn_test_poison_workspace fills it); what follows is not
    c->scal = (float*)bump(p, 256);
    c->zero_page = (bf16_t*)bump(p, WN_ZERO_PAGE_BYTES);
    c->score_part = (double*)bump(p, (size_t)wn_score_part_doubles(c->maxB, c->maxT) * 8);
    if (hipMemset(c->zero_page, 0, WN_ZERO_PAGE_BYTES) != hipSuccess) WN_FAIL(c, WN_E_HIP, "hipMemset(zero page) failed");
    return WN_OK;
}

static int stream_alloc(wn_ctx* c);

extern "C" int wn_create(const wn_config* cfg, wn_ctx** out) {
    wn_ctx* z = nullptr;
    if (!cfg || !out) WN_FAIL(z, WN_E_ARG, "wn_create: null argument");
    if (cfg->abi_version != WN_ABI_VERSION) WN_FAIL(z, WN_E_ARG, "wn_create: abi_version %d != %d", cfg->abi_version, WN_ABI_VERSION);
    // constraints enforced by the reference
    if (cfg->layers <= 0 || cfg->stacks <= 0 || cfg->layers % cfg->stacks != 0)
        WN_FAIL(z, WN_E_SHAPE, "layers (%d) must be a positive multiple of stacks (%d) [wavenet.py:97]", cfg->layers, cfg->stacks);
    if (cfg->kernel_size != 3) WN_FAIL(z, WN_E_UNSUPPORTED, "kernel_size %d: only 3 is built", cfg->kernel_size);
    if (cfg->input_type < 0 || cfg->input_type > 2) WN_FAIL(z, WN_E_ARG, "bad input_type %d [util.py:10-11]", cfg->input_type);
    if (cfg->input_type == WN_INPUT_MULAW_QUANTIZE && cfg->out_channels != cfg->quantize_channels)
        WN_FAIL(z, WN_E_SHAPE, "out_channels must equal to quantize_chennels if input_type is 'mulaw-quantize' [models/__init__.py:6-9]");
    if (cfg->input_type != WN_INPUT_MULAW_QUANTIZE && cfg->out_channels != 2 && cfg->out_channels % 3 != 0)
        WN_FAIL(z, WN_E_SHAPE, "out_channels (%d) must be 2 (Gaussian) or a multiple of 3 (MoL) [mixture.py:30]", cfg->out_channels);
    if (cfg->gate_channels % 2) WN_FAIL(z, WN_E_SHAPE, "gate_channels must be even");
    if (cfg->residual_channels % 64 || (cfg->gate_channels / 2) % 32 || cfg->skip_out_channels % 64 || cfg->gate_channels % 64)
        WN_FAIL(z, WN_E_UNSUPPORTED, "channel counts must be multiples of 64 (R=%d G=%d S=%d) for the MFMA tiling",
                cfg->residual_channels, cfg->gate_channels, cfg->skip_out_channels);
    if (cfg->cin_channels <= 0 || cfg->cin_channels % 16)
        WN_FAIL(z, WN_E_UNSUPPORTED, "cin_channels (%d) must be a positive multiple of 16 (local conditioning is required)", cfg->cin_channels);
    if (cfg->gin_channels > 0 && cfg->use_speaker_embedding && cfg->n_speakers <= 0)
        WN_FAIL(z, WN_E_ARG, "n_speakers must be positive when use_speaker_embedding [wavenet.py:154]");
    if (cfg->gin_channels > 256) WN_FAIL(z, WN_E_UNSUPPORTED, "gin_channels > 256");
    if (cfg->n_upsample < 0 || cfg->n_upsample > WN_MAX_UPSAMPLE) WN_FAIL(z, WN_E_ARG, "bad n_upsample");
    if (cfg->upsample_type != WN_UP_NEAREST && cfg->upsample_type != WN_UP_2D && cfg->upsample_type != WN_UP_SUBPIXEL &&
        cfg->upsample_type != WN_UP_1D && cfg->upsample_type != WN_UP_RESIZE)
        WN_FAIL(z, WN_E_ARG, "bad upsample_type %d", cfg->upsample_type);
    if (cfg->freq_axis_kernel_size % 2 == 0 || cfg->freq_axis_kernel_size > 9) WN_FAIL(z, WN_E_UNSUPPORTED, "freq_axis_kernel_size must be odd <= 9");
    if (cfg->max_batch <= 0 || cfg->max_time <= 0) WN_FAIL(z, WN_E_ARG, "max_batch/max_time must be positive");
    if (cfg->dropout < 0.f || cfg->dropout >= 1.f) WN_FAIL(z, WN_E_ARG, "dropout must be in [0,1)");
    if (cfg->compute_dtype != WN_COMPUTE_BF16 && cfg->compute_dtype != WN_COMPUTE_F32) WN_FAIL(z, WN_E_ARG, "bad compute_dtype %d", cfg->compute_dtype);
    int hop = 1; for (int i = 0; i < cfg->n_upsample; ++i) { if (cfg->upsample_scales[i] <= 0) WN_FAIL(z, WN_E_ARG, "bad upsample scale"); hop *= cfg->upsample_scales[i]; }

    wn_ctx* c = new wn_ctx();
    c->cfg = *cfg;
    c->L = cfg->layers; c->R = cfg->residual_channels; c->G = cfg->gate_channels; c->GH = c->G / 2;
    c->S = cfg->skip_out_channels; c->O = cfg->out_channels; c->C = cfg->cin_channels;
    c->Cin = (cfg->input_type == WN_INPUT_MULAW_QUANTIZE) ? cfg->quantize_channels : 1;
    c->hop = hop;
    c->lbias = cfg->use_bias != 0;
    c->wnorm = cfg->weight_normalization != 0;
    c->inference = cfg->inference_only != 0;
    c->pipe_f16 = WN_PIPE_F16_DEFAULT;
    if (const char* ed = getenv("WN_PIPE_DTYPE")) {      // case-insensitive; an unknown spelling is an error, not a silent bf16
        std::string v(ed); for (char& ch : v) ch = (char)tolower((unsigned char)ch);
        if (v == "fp16" || v == "f16" || v == "half" || v == "float16") c->pipe_f16 = true;
        else if (v == "bf16" || v == "bfloat16") c->pipe_f16 = false;
        else { delete c; WN_FAIL(z, WN_E_ARG, "WN_PIPE_DTYPE='%s': expected fp16 (f16, half, float16) or bf16 (bfloat16)", ed); }
    }
    { const char* e8 = getenv("WN_GEMM8P"); c->gemm8p = e8 ? atoi(e8) : 0; }      // bit 0: gate, bit 1: d x on the 8-phase kernel (wn_tile8p.h; measured: not faster on any shipped workload)
    { const char* e16 = getenv("WN_MFMA16"); c->mfma16 = (e16 ? atoi(e16) : WN_MFMA16_DEFAULT) & WN_MF16_ALL; }      // MFMA shape per launch kind of the ring kernel (wn_tile.h); unset: the kinds that won
    c->gin = cfg->gin_channels > 0 ? cfg->gin_channels : 0;
    c->OP = (int)align_up(c->O, 32); c->CP = (int)align_up(c->C, 32);
    const int per = c->L / cfg->stacks;
    for (int l = 0; l < c->L; ++l) c->dil.push_back(1 << (l % per));             // wavenet.py:125
    c->res_scale = cfg->residual_legacy ? WN_SQRT_HALF : 1.0f;
    c->skip_scale.resize(c->L);
    for (int l = 0; l < c->L; ++l) {                                             // wavenet.py:706-715 unrolled
        int e = cfg->legacy ? (l == 0 ? c->L - 1 : c->L - l) : 0;
        c->skip_scale[l] = (float)pow((double)WN_SQRT_HALF, e);
    }
    build_layout(c);
    wn_plan_buckets(c);
    c->cup_final_idx = (cfg->upsample_type == WN_UP_NEAREST) ? 0 : cfg->n_upsample - 1;
    c->maxB = cfg->max_batch; c->maxT = cfg->max_time; c->NT = (int64_t)c->maxB * c->maxT;
    int rc = alloc_workspace(c);
    if (rc == WN_OK) rc = wn_build_packs(c);
    if (rc == WN_OK && !c->inference) {
        const size_t need = wn_wgrad_partial_need(c);
        rc = [&]() -> int { WN_HIP(c, c->wg_partial.reserve(need / 4)); return WN_OK; }();
    }
    if (rc == WN_OK && c->inference) {
        // pre-size every synthesis buffer for (max_batch, max_time): wn_synthesize never allocates on this context.  The pipeline, the streaming state and the
        // narrow slot sessions serve at most 32 streams and are sized for nb = min(32, max_batch); a larger max_batch adds the state of wn_synthesize_wide and
        // the tables of a wide slot session (wn_synth_wide_slots_begin) for all of it
        const int nb = std::min(32, c->maxB);
        if (rc == WN_OK) rc = wn_noise_reserve(c, c->maxB, c->maxT);
        // the persistent pipeline when the model fits it, pre-sized for the LARGEST eligible run of <= max_batch streams (it was
        // sized for max_batch or else 8, so a batch between 8 and a non-eligible max_batch was eligible by wn_synth_pipe_eligible and then
        // failed to grow); else the launch-per-layer graph path
        if (rc == WN_OK) {
            int pb = nb;
            while (pb > 0 && !wn_pipe_eligible(c, pb)) --pb;
            c->pipe_cap = pb;
            rc = c->cfg.compute_dtype == WN_COMPUTE_F32 ? wn_synth_f32_reserve(c, nb) : pb > 0 ? wn_pipe_reserve(c, pb, c->maxT) : wn_synth_reserve(c);
        }
        if (rc == WN_OK && c->maxB > 32 && c->cfg.compute_dtype != WN_COMPUTE_F32) rc = wn_synth_wide_reserve(c, c->maxB);
        if (rc == WN_OK) rc = stream_alloc(c);      // the streaming state too: wn_synth_stream_* never allocate here
        if (rc == WN_OK && c->cfg.compute_dtype != WN_COMPUTE_F32) rc = wn_slots_alloc(c, c->maxB > 32 ? c->maxB : nb);      // ... nor do wn_synth_slots_*, wn_synth_wide_slots_begin and wn_synthesize_folded
    }
    if (rc != WN_OK) { g_create_err = c->err; wn_destroy(c); return rc; }
    *out = c;
    return WN_OK;
}

// Every device resource is released by its owner's destructor (wn_dev.h).  The context's own streams are drained first, so that nothing of ours still
// runs when the buffers go; the per-path states (declared last in wn_ctx) then drain and destroy their private streams before any buffer is freed.
extern "C" void wn_destroy(wn_ctx* c) {
    if (!c) return;
    for (hipStream_t st : c->stp) if (st) (void)hipStreamSynchronize(st);      // (stp[1] is st2)
    if (c->st3) (void)hipStreamSynchronize(c->st3);
    delete c;
}

extern "C" const char* wn_last_error(const wn_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }
extern "C" int wn_receptive_field(const wn_ctx* c) { if (!c) return WN_E_ARG; int s = 0; for (int d : c->dil) s += d; return 2 * s + 1; }
extern "C" int64_t wn_param_count(const wn_ctx* c) { return c ? c->n_raw : (int64_t)WN_E_ARG; }
extern "C" int wn_num_tensors(const wn_ctx* c) { return c ? (int)c->raw_tensors.size() : WN_E_ARG; }
extern "C" int wn_tensor_info(const wn_ctx* c, int i, char* name, int32_t* shape, int32_t* ndim, int64_t* offset) {
    if (!c || i < 0 || i >= (int)c->raw_tensors.size()) return WN_E_ARG;
    const WnTensor& t = c->raw_tensors[i];
    if (name) { strncpy(name, t.name.c_str(), 127); name[127] = 0; }
    if (shape) for (int k = 0; k < 4; ++k) shape[k] = t.shape[k];
    if (ndim) *ndim = t.ndim;
    if (offset) *offset = t.offset;
    return WN_OK;
}
extern "C" int64_t wn_workspace_bytes(const wn_ctx* c) { return c ? (int64_t)(c->ws.bytes() + c->wg_partial.bytes()) : (int64_t)WN_E_ARG; }
extern "C" const char* wn_dominant_kernel_name(void) {      // the gate launch of a context created without WN_MFMA16 (last template argument: the MFMA shape)
    return (WN_MFMA16_DEFAULT & WN_MF16_GATE) ? "wn_gemm_lds_kernel<2, 2, 4, 2, 32, 3, 0, 1, 3, 1>" : "wn_gemm_lds_kernel<2, 2, 4, 2, 32, 3, 0, 1, 3, 0>";
}

// rocTX ranges around the host side of the drop-in entry points (tracing): `rocprofv3 --marker-trace --kernel-trace` then
// shows which call enqueued which kernels.  The marker library is looked up at run time (dlopen of libroctx64.so / the SDK's
// librocprofiler-sdk-roctx.so; no link dependency) and only when WN_ROCTX=1: otherwise a range costs one predictable branch.
struct WnRoctx {
    int (*push)(const char*) = nullptr; int (*pop)() = nullptr;
    WnRoctx() {
        const char* e = getenv("WN_ROCTX");
        if (!e || atoi(e) == 0) return;
        for (const char* name : {"librocprofiler-sdk-roctx.so", "libroctx64.so", "/opt/rocm/lib/librocprofiler-sdk-roctx.so", "/opt/rocm/lib/libroctx64.so"}) {
            void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (!h) continue;
            push = (int (*)(const char*))dlsym(h, "roctxRangePushA"); pop = (int (*)())dlsym(h, "roctxRangePop");
            if (push && pop) return;
            push = nullptr; pop = nullptr;
        }
    }
};
static WnRoctx& wn_roctx() { static WnRoctx r; return r; }
struct WnRange {
    bool on;
    explicit WnRange(const char* name) : on(wn_roctx().push != nullptr) { if (on) wn_roctx().push(name); }
    ~WnRange() { if (on) wn_roctx().pop(); }
};

extern "C" int wn_pack_weights(wn_ctx* c, const float* params, void* stream) {
    if (!c || !params) return WN_E_ARG;
    WnRange range("wn_pack_weights");
    c->strm.open = false; c->slots.open = false;       // (ends an open stream / slot session: its pipeline slices / bias are of the old weights)
    return wn_launch_pack(c, params, (hipStream_t)stream);
}

extern "C" float wn_learning_rate(int32_t schedule, float init_lr, int64_t step, float decay_rate,
                                  int64_t decay_steps, float warmup) {
    if (schedule == WN_LR_NOAM) {                                   // wavenet.py:615-618
        double s = (double)(step + 1);
        double v = init_lr * pow((double)warmup, 0.5) * fmin(s * pow((double)warmup, -1.5), pow(s, -0.5));
        return (float)fmax(v, 1e-4);
    }
    return (float)(init_lr * pow((double)decay_rate, (double)step / (double)decay_steps));   // wavenet.py:620-629
}

extern "C" int wn_set_global_condition(wn_ctx* c, const void* g, int32_t B, void* stream) {
    if (!c || !g) return WN_E_ARG;
    if (c->gin <= 0) WN_FAIL(c, WN_E_STATE, "wn_set_global_condition: the model has no global conditioning (gin_channels <= 0)");
    if (B <= 0 || B > c->maxB) WN_FAIL(c, WN_E_SHAPE, "batch %d outside (0, max_batch=%d]", B, c->maxB);
    c->strm.open = false;
    if (c->cfg.use_speaker_embedding) WN_HIP(c, hipMemcpyAsync(c->gids, g, (size_t)B * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    else WN_HIP(c, hipMemcpyAsync(c->gvec, g, (size_t)B * c->gin * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    c->gB = B; c->have_g = true;
    return WN_OK;
}

static int check_fwd_args(wn_ctx* c, const void* x, const float* cc, const void* y, const int32_t* len, int B, int T, int Tc) {
    if (!x || !cc || !y || !len) WN_FAIL(c, WN_E_ARG, "wn_train_fwd: null pointer (Please provide either lengths or mask [modules.py:782-783])");
    if (B <= 0 || B > c->maxB) WN_FAIL(c, WN_E_SHAPE, "batch %d outside (0, max_batch=%d]", B, c->maxB);
    if (T <= 1 || T > c->maxT) WN_FAIL(c, WN_E_SHAPE, "time %d outside (1, max_time=%d]", T, c->maxT);
    if (Tc * c->hop != T) WN_FAIL(c, WN_E_SHAPE, "upsampled conditioning length Tc*hop = %d*%d != T = %d [wavenet.py:699]", Tc, c->hop, T);
    if (!c->packed) WN_FAIL(c, WN_E_STATE, "wn_pack_weights must be called before wn_train_fwd");
    if (c->gin > 0 && (!c->have_g || c->gB != B))
        WN_FAIL(c, WN_E_STATE, "global conditioning is enabled: call wn_set_global_condition with this batch (B=%d) first [wavenet.py:669-678]", B);
    return WN_OK;
}

extern "C" int wn_train_fwd(wn_ctx* c, const void* x, const float* cc, const void* y, const int32_t* lengths,
                            int32_t B, int32_t T, int32_t Tc, uint64_t seed, float* loss_out, float* y_hat_out, void* stream) {
    if (!c) return WN_E_ARG;
    WnRange range("wn_train_fwd");
    if (c->inference) WN_FAIL(c, WN_E_STATE, "wn_train_fwd on an inference-only context (cfg.inference_only = 1)");
    int rc = check_fwd_args(c, x, cc, y, lengths, B, T, Tc);
    if (rc) return rc;
    // x and c are needed again by wn_train_bwd: keep ctx-owned copies (caller pointers are borrowed for this call only)
    WN_HIP(c, hipMemcpyAsync(c->XIN, x, (size_t)B * T * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    WN_HIP(c, hipMemcpyAsync(c->CIN, cc, (size_t)B * c->C * Tc * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    c->fx = c->XIN; c->fc = c->CIN; c->fy = y; c->flen = lengths; c->fB = B; c->fT = T; c->fTc = Tc; c->fseed = seed; c->fup_pitch = 0;
    c->have_fwd = false; c->have_bwd = false;
    rc = wn_fwd_impl(c, (hipStream_t)stream, loss_out, y_hat_out);
    if (rc == WN_OK) c->have_fwd = true;
    return rc;
}

// Evaluation: the teacher-forced forward without dropout + per-utterance / per-sample scores.  x and c are read in stream order during this call's
// launches only (no ctx-owned copies: nothing is kept for a backward), so wn_train_bwd afterwards is refused until the next wn_train_fwd.
extern "C" int wn_eval_fwd(wn_ctx* c, const void* x, const float* cc, const void* y, const int32_t* lengths, int32_t B, int32_t T, int32_t Tc,
                           float* stats_out, float* nll_out, float* y_hat_out, void* stream) {
    if (!c) return WN_E_ARG;
    WnRange range("wn_eval_fwd");
    if (c->inference) WN_FAIL(c, WN_E_STATE, "wn_eval_fwd on an inference-only context (cfg.inference_only = 1)");
    int rc = check_fwd_args(c, x, cc, y, lengths, B, T, Tc);
    if (rc) return rc;
    if (!stats_out) WN_FAIL(c, WN_E_ARG, "wn_eval_fwd: stats_out is NULL");
    c->fx = x; c->fc = cc; c->fy = y; c->flen = lengths; c->fB = B; c->fT = T; c->fTc = Tc; c->fseed = 0; c->fup_pitch = 0;
    c->have_fwd = false; c->have_bwd = false; c->have_loss = false;
    rc = wn_fwd_impl(c, (hipStream_t)stream, nullptr, y_hat_out, true);
    c->feval = false; c->fx = c->XIN; c->fc = c->CIN;      // (the borrowed pointers are in the launches; none is kept)
    if (rc) return rc;
    return wn_score_last_fwd(c, stats_out, nll_out, (hipStream_t)stream);
}

extern "C" int wn_train_bwd(wn_ctx* c, float* grads, void* stream) {
    if (!c || !grads) return WN_E_ARG;
    WnRange range("wn_train_bwd");
    if (!c->have_fwd) WN_FAIL(c, WN_E_STATE, "wn_train_bwd called without a preceding successful wn_train_fwd");
    return wn_bwd_impl(c, grads, (hipStream_t)stream);
}

extern "C" int wn_optim_step(wn_ctx* c, float* p, const float* g, float* m, float* v, float* ema, float lr, int64_t step, void* stream) {
    if (!c || !p || !g || !m || !v || !ema) return WN_E_ARG;
    WnRange range("wn_optim_step");
    if (c->inference) WN_FAIL(c, WN_E_STATE, "wn_optim_step on an inference-only context (cfg.inference_only = 1)");
    return wn_optim_impl(c, p, g, m, v, ema, lr, step, (hipStream_t)stream);
}

extern "C" int wn_get_upsampled_features(wn_ctx* c, float* out, void* stream) {
    if (!c || !out) return WN_E_ARG;
    if (c->fB <= 0) WN_FAIL(c, WN_E_STATE, "no forward/synthesis has run yet");
    if (c->fup_pitch < 0)      // after a push of a slot session: [B][C][n_max], row b = the rows slot b's steps of that push read (rows of slots that generated fewer: stale beyond their count)
        WN_HIP(c, hipMemcpyAsync(out, c->slots.feat, (size_t)c->slots.feat_B * c->C * c->slots.feat_pitch * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    else if (c->fup_pitch > 0)      // after a stream push: the span's columns of the upsampled window
        WN_HIP(c, hipMemcpy2DAsync(out, (size_t)c->fT * 4, c->CUP[c->cup_final_idx] + c->fup_off, (size_t)c->fup_pitch * 4, (size_t)c->fT * 4, (size_t)c->fB * c->C,
                                   hipMemcpyDeviceToDevice, (hipStream_t)stream));
    else WN_HIP(c, hipMemcpyAsync(out, c->CUP[c->cup_final_idx], (size_t)c->fB * c->C * c->fT * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return WN_OK;
}

extern "C" int wn_synthesize(wn_ctx* c, const float* cc, int32_t B, int32_t Tc, const float* noise, uint64_t seed,
                             const void* test_inputs, void* out_samples, float* out_raw, int32_t steps_per_graph, void* stream) {
    if (!c || !cc || !out_samples) return WN_E_ARG;
    WnRange range("wn_synthesize");
    if (!c->packed) WN_FAIL(c, WN_E_STATE, "wn_pack_weights must be called before wn_synthesize");
    if (B <= 0 || B > 32) WN_FAIL(c, WN_E_SHAPE, "synthesis batch %d outside (0, 32]", B);
    if (Tc <= 0) WN_FAIL(c, WN_E_SHAPE, "Tc must be positive");
    c->strm.open = false; c->slots.open = false;            // (ends an open stream / slot session: its queues are overwritten)
    int rc = wn_pipe_check(c, false);                  // a hand-off timeout of the previous pipeline run surfaces here at the latest
    if (rc) return rc;
    const bool tempered = c->tau_scale != 1.0f || c->tau_select != 1.0f;
    if (!noise || tempered) {                          // device Philox stream keyed by `seed` (header), generated already tempered; or the tempered copy of the caller's noise
        const int T = Tc * c->hop;
        if ((rc = wn_noise_reserve(c, B, T))) return rc;
        if ((rc = noise ? wn_temper_noise_impl(c, noise, c->noise_buf, B, T, c->tau_scale, c->tau_select, (hipStream_t)stream)
                        : wn_fill_noise_impl(c, c->noise_buf, B, T, seed, c->tau_scale, c->tau_select, (hipStream_t)stream))) return rc;
        noise = c->noise_buf;
    }
    return wn_synth_impl(c, cc, B, Tc, noise, seed, test_inputs, out_samples, out_raw, steps_per_graph, (hipStream_t)stream);
}

// The launch-per-layer run of wn_synthesize(steps_per_graph > 0) for any 0 < B <= max_batch: ceil(B / 32) tiles of streams per launch (wn_synth.hip).
extern "C" int wn_synthesize_wide(wn_ctx* c, const float* cc, int32_t B, int32_t Tc, const float* noise, uint64_t seed,
                                  const void* test_inputs, void* out_samples, float* out_raw, int32_t steps_per_graph, void* stream) {
    if (!c || !cc || !out_samples) return WN_E_ARG;
    WnRange range("wn_synthesize_wide");
    if (c->cfg.compute_dtype == WN_COMPUTE_F32) WN_FAIL(c, WN_E_UNSUPPORTED, "wn_synthesize_wide: wide runs are not built for the fp32 validation mode (compute_dtype = WN_COMPUTE_F32)");
    if (!c->packed) WN_FAIL(c, WN_E_STATE, "wn_pack_weights must be called before wn_synthesize_wide");
    if (B <= 0 || B > c->maxB) WN_FAIL(c, WN_E_SHAPE, "wide synthesis batch %d outside (0, max_batch = %d]", B, c->maxB);
    if (Tc <= 0) WN_FAIL(c, WN_E_SHAPE, "Tc must be positive");
    const int64_t T64 = (int64_t)Tc * c->hop;
    if (T64 * B > c->NT) WN_FAIL(c, WN_E_SHAPE, "synthesis B*T = %d*%lld exceeds the workspace (max_batch*max_time = %lld)", B, (long long)T64, (long long)c->NT);
    c->strm.open = false; c->slots.open = false;            // (ends an open stream / slot session, as wn_synthesize does)
    int rc = wn_pipe_check(c, false);
    if (rc) return rc;
    const int T = (int)T64;      // (<= NT / B: the kernels index [T][B][nps], [B][O][T] and the queues in 64 bits, so no further shape is refused)
    const bool tempered = c->tau_scale != 1.0f || c->tau_select != 1.0f;
    if (!noise || tempered) {
        if ((rc = wn_noise_reserve(c, B, T))) return rc;
        if ((rc = noise ? wn_temper_noise_impl(c, noise, c->noise_buf, B, T, c->tau_scale, c->tau_select, (hipStream_t)stream)
                        : wn_fill_noise_impl(c, c->noise_buf, B, T, seed, c->tau_scale, c->tau_select, (hipStream_t)stream))) return rc;
        noise = c->noise_buf;
    }
    return wn_synth_impl(c, cc, B, Tc, noise, seed, test_inputs, out_samples, out_raw, steps_per_graph, (hipStream_t)stream, true);
}

extern "C" int wn_fill_noise(wn_ctx* c, float* noise, int32_t B, int32_t T, uint64_t seed, void* stream) {
    if (!c || !noise || B <= 0 || T <= 0) return WN_E_ARG;
    return wn_fill_noise_impl(c, noise, B, T, seed, 1.0f, 1.0f, (hipStream_t)stream);      // untempered: the documented way to reproduce a device-noise run (wn_temper_noise)
}

// ---- sampling temperature (wn_temper.h): host state of the context / of a live slot; the noise kernels do the work
static int tau_check(wn_ctx* c, const char* who, float tau_scale, float tau_select) {
    if (!wn_tau_valid(tau_scale) || !wn_tau_valid(tau_select))
        WN_FAIL(c, WN_E_ARG, "%s: temperatures (%g, %g) must be finite and in [0, 2]", who, (double)tau_scale, (double)tau_select);
    return WN_OK;
}
extern "C" int wn_synth_set_temperature(wn_ctx* c, float tau_scale, float tau_select) {
    if (!c) return WN_E_ARG;
    int rc = tau_check(c, "wn_synth_set_temperature", tau_scale, tau_select);
    if (rc) return rc;
    c->tau_scale = tau_scale; c->tau_select = tau_select;
    return WN_OK;
}
extern "C" int wn_synth_get_temperature(const wn_ctx* c, float* tau_scale, float* tau_select) {
    if (!c || !tau_scale || !tau_select) return WN_E_ARG;
    *tau_scale = c->tau_scale; *tau_select = c->tau_select;
    return WN_OK;
}
extern "C" int wn_temper_noise(wn_ctx* c, const float* in, float* out, int32_t B, int32_t T, float tau_scale, float tau_select, void* stream) {
    if (!c) return WN_E_ARG;
    if (!in || !out || B <= 0 || T <= 0) WN_FAIL(c, WN_E_ARG, "wn_temper_noise: null buffer or B = %d, T = %d not positive", B, T);
    int rc = tau_check(c, "wn_temper_noise", tau_scale, tau_select);
    if (rc) return rc;
    return wn_temper_noise_impl(c, in, out, B, T, tau_scale, tau_select, (hipStream_t)stream);
}
extern "C" int wn_test_fill_noise_tempered(wn_ctx* c, float* noise, int32_t B, int32_t T, uint64_t seed, float tau_scale, float tau_select, void* stream) {
    if (!c || !noise || B <= 0 || T <= 0) return WN_E_ARG;
    int rc = tau_check(c, "wn_test_fill_noise_tempered", tau_scale, tau_select);
    if (rc) return rc;
    return wn_fill_noise_impl(c, noise, B, T, seed, tau_scale, tau_select, (hipStream_t)stream);
}
// test hook: the same function on the host (no context, no GPU)
extern "C" int wn_test_temper_noise(int32_t mode, int32_t nps, const float* in, float* out, int64_t rows, float tau_scale, float tau_select) {
    if (!in || !out || rows < 0 || mode < 0 || mode > 2 || nps < 1 || !wn_tau_valid(tau_scale) || !wn_tau_valid(tau_select)) return WN_E_ARG;
    for (int64_t r = 0; r < rows; ++r)
        for (int q = 0; q < nps; ++q) out[r * nps + q] = wn_temper_entry(in[r * nps + q], mode, nps, q, tau_scale, tau_select);
    return WN_OK;
}
extern "C" int wn_synth_check(wn_ctx* c) { if (!c) return WN_E_ARG; return wn_pipe_check(c, true); }
extern "C" int wn_synth_last_path(const wn_ctx* c) { return c ? c->synth_path : WN_E_ARG; }
extern "C" int wn_synth_last_instances(const wn_ctx* c) { return c ? c->synth_instances : WN_E_ARG; }
extern "C" int wn_synth_last_batched(const wn_ctx* c) { return c ? (c->synth_path == 2 ? c->synth_batchpre : 0) : WN_E_ARG; }
extern "C" int wn_synth_pipe_dtype(wn_ctx* c, int32_t half) { if (!c) return WN_E_ARG; c->pipe_f16 = half != 0; c->strm.open = false; c->slots.open = false; return WN_OK; }
extern "C" int wn_synth_last_config(const wn_ctx* c, int32_t* out, int32_t cap) {
    if (!c || !out || cap < 0) return WN_E_ARG;
    int32_t v[WN_SYNTH_CFG_N] = {c->synth_path, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (c->synth_path == 2) for (int i = 1; i < WN_SYNTH_CFG_N; ++i) v[i] = c->synth_cfg[i];
    const int n = cap < WN_SYNTH_CFG_N ? cap : WN_SYNTH_CFG_N;
    for (int i = 0; i < n; ++i) out[i] = v[i];
    return n;
}
extern "C" int wn_test_gemm8p_mask(const wn_ctx* c) {
    if (!c) return WN_E_ARG;
    if (c->packs.empty()) return 0;
    return (c->packs[0].w1.kil == 64 ? 1 : 0) | (c->packs[0].w1T.kil == 64 ? 2 : 0);
}
extern "C" int wn_test_mfma16_mask(const wn_ctx* c) { return c ? c->mfma16 : WN_E_ARG; }
// Every byte a training step may find from an earlier one becomes 0xFF (a NaN in bf16 and in fp32), over the whole allocations: the step-owned front of
// the workspace (cbt, X, XD, TS, U, R1, H2, DY, DPRE1, DSKIP, DZ, GXall, YHAT, DC, CUP[], DCUP[], UPPART, XIN, CIN, cs_part), the split-K partials of the
// grouped weight gradients, the effective-gradient buffer, the per-step global-conditioning tables (gbias, colsum) and the fp32 mode's state.  Memsets in
// stream order only.  Not touched: scal, zero_page and score_part behind that front, parameters, packs, b1sum, the skip-bias total, gvec / gids, every
// integer table, profiling and trace state, and all synthesis / stream / slot state.
extern "C" int wn_test_poison_workspace(wn_ctx* c, void* stream) {
    if (!c) return WN_E_ARG;
    if (c->inference) WN_FAIL(c, WN_E_STATE, "wn_test_poison_workspace: no training workspace on an inference-only context");
    hipStream_t st = (hipStream_t)stream;
    c->have_fwd = false; c->have_bwd = false; c->have_loss = false;      // nothing of the last step is left to run a backward on
    WN_HIP(c, hipMemsetAsync(c->ws.get(), 0xFF, c->ws_step_bytes, st));
    if (c->wg_partial) WN_HIP(c, hipMemsetAsync(c->wg_partial.get(), 0xFF, c->wg_partial.bytes(), st));
    if (c->deff) WN_HIP(c, hipMemsetAsync(c->deff.get(), 0xFF, c->deff.bytes(), st));
    if (c->gbias) WN_HIP(c, hipMemsetAsync(c->gbias.get(), 0xFF, c->gbias.bytes(), st));
    if (c->colsum) WN_HIP(c, hipMemsetAsync(c->colsum.get(), 0xFF, c->colsum.bytes(), st));
    return wn_f32_poison(c, st);
}
extern "C" int wn_synth_pipe_eligible(const wn_ctx* c, int32_t B) {
    if (!c || B <= 0) return WN_E_ARG;
    const char* m = getenv("WN_SYNTH_MODE");
    if (m && strcmp(m, "graph") == 0) return 0;
    if (c->inference && c->pipe_cap > 0 && B > c->pipe_cap) return 0;      // an inference-only context never grows its pipeline: larger batches go in groups
    return wn_pipe_eligible(c, B) ? 1 : 0;
}

int wn_noise_reserve(wn_ctx* c, int B, int T) {
    const size_t need = (size_t)B * T * wn_noise_per_step(c) * 4;
    if (need <= c->noise_buf.bytes()) return WN_OK;
    if (c->inference && c->noise_buf) WN_FAIL(c, WN_E_SHAPE, "synthesis B*T = %d*%d exceeds the pre-sized noise buffer of this inference-only context", B, T);
    if (c->noise_buf) (void)hipDeviceSynchronize();      // (growing: nothing may still read the old buffer)
    WN_HIP(c, c->noise_buf.grow(need / 4));
    return WN_OK;
}

extern "C" int wn_noise_per_step(const wn_ctx* c) {
    if (!c) return WN_E_ARG;
    if (c->cfg.input_type == WN_INPUT_MULAW_QUANTIZE) return c->cfg.quantize_channels;
    if (c->O == 2) return 1;
    return c->O / 3 + 1;
}

extern "C" int wn_sample(wn_ctx* c, const float* y_hat, int32_t B, int32_t T, const float* noise, void* out, void* stream) {
    if (!c || !y_hat || !noise || !out) return WN_E_ARG;
    return wn_sample_impl(c, y_hat, B, T, noise, out, (hipStream_t)stream);
}

// ---- debug access to internal activations (tests only; converts bf16 buffers to fp32) --------
__global__ void wn_bf16_to_f32(const bf16_t* __restrict__ in, float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = bf2f(in[i]);
}
extern "C" int wn_debug_copy(wn_ctx* c, const char* name, int32_t layer, float* out, int64_t n, void* stream) {
    if (!c || !name || !out || n <= 0) return WN_E_ARG;
    {   // the weight path: the context's own parameter copy, the effective-kernel gradients and the two bias sums (sized buffers: n is checked)
        const std::string w = name;
        const float* src = nullptr; int64_t len = 0;
        if (w == "PARAMS") { src = c->params_dev; len = c->n_params; }
        else if (w == "B1SUM") { src = c->b1sum; len = (int64_t)c->L * c->G; }
        else if (w == "SKIPB") { src = c->skip_bias_total; len = c->S; }
        else if (w == "DEFF") {
            if (!c->wnorm) WN_FAIL(c, WN_E_STATE, "wn_debug_copy('DEFF'): the context has no weight normalisation (the gradients of wn_train_bwd are the effective ones)");
            if (!c->have_bwd) WN_FAIL(c, WN_E_STATE, "wn_debug_copy('DEFF'): no wn_train_bwd has run since the last forward");
            src = c->deff; len = c->n_params;
        }
        if (src) {
            if (!c->packed) WN_FAIL(c, WN_E_STATE, "wn_debug_copy('%s'): wn_pack_weights has not run yet", name);
            if (n > len) WN_FAIL(c, WN_E_ARG, "wn_debug_copy('%s'): n = %lld exceeds the buffer's %lld floats", name, (long long)n, (long long)len);
            WN_HIP(c, hipMemcpyAsync(out, src, (size_t)n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
            return WN_OK;
        }
    }
    if (c->inference && strcmp(name, "cbt") != 0 && strcmp(name, "CUP") != 0) WN_FAIL(c, WN_E_STATE, "wn_debug_copy('%s'): no training workspace on an inference-only context", name);
    const int64_t NT = c->NT;
    const bf16_t* b = nullptr; const float* f = nullptr;
    std::string s = name;
    if (c->cfg.compute_dtype == WN_COMPUTE_F32 && (s == "X" || s == "U" || s == "Z" || s == "SK" || s == "H1")) {
        if (layer < 0 || layer >= c->L) WN_FAIL(c, WN_E_ARG, "wn_debug_copy('%s'): layer %d outside [0, %d)", name, layer, c->L);
        f = wn_f32_debug(c, name, layer);
        if (!f) WN_FAIL(c, WN_E_STATE, "wn_debug_copy('%s'): no fp32 forward has run yet", name);
    }
    else if (s == "cbt") b = c->cbt;
    else if (s == "X") b = c->X + (size_t)layer * NT * c->R;
    else if (s == "TS") b = c->TS + (size_t)layer * NT * c->GH;      // sigmoid [rows][G/2]
    else if (s == "U") b = c->U + (size_t)layer * NT * c->GH;
    else if (s == "R1") b = c->R1;
    else if (s == "H2") b = c->H2;
    else if (s == "DY") b = c->DY;
    else if (s == "DPRE1") b = c->DPRE1;
    else if (s == "DSKIP") b = c->DSKIP;
    else if (s == "DZ") b = c->DZ + (size_t)layer * NT * c->G;
    else if (s == "GX0") b = c->GX0;
    else if (s == "GX1") b = c->GX1;
    else if (s == "GX" || s == "XD") {      // d L / d h_layer (layer L: the zero-filled top) / the dropout-applied conv input (aliases X when dropout is 0)
        const int hi = s == "GX" ? c->L : c->L - 1;
        if (layer < 0 || layer > hi) WN_FAIL(c, WN_E_ARG, "wn_debug_copy('%s'): layer %d outside [0, %d]", name, layer, hi);
        b = (s == "GX" ? c->GXall : c->XD) + (size_t)layer * NT * c->R;
    }
    else if (s == "YHAT") f = c->YHAT;
    else if (s == "DC") f = c->DC;
    else if (s == "CUP") f = c->CUP[layer];
    else WN_FAIL(c, WN_E_ARG, "wn_debug_copy: unknown buffer '%s'", name);
    hipStream_t st = (hipStream_t)stream;
    if (b) { hipLaunchKernelGGL(wn_bf16_to_f32, dim3(cdiv(n, 256)), dim3(256), 0, st, b, out, n); WN_LAUNCH_CHECK(c); }
    else WN_HIP(c, hipMemcpyAsync(out, f, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    return WN_OK;
}

// ---- test hooks: the fragment-ordered bf16 packs as wn_pack_kernel stored them (no un-shuffling)
static const PackedW* find_pack(const wn_ctx* c, const char* kind, int32_t layer, bool* per_layer) {
    const std::string k = kind;
    static const char* const lay[5] = {"w1", "wo", "ws", "w2T", "w1T"};
    *per_layer = false;
    for (int i = 0; i < 5; ++i) if (k == lay[i]) {
        *per_layer = true;
        if (layer < 0 || layer >= (int)c->packs.size()) return nullptr;
        const WnLayerPacks& p = c->packs[layer];
        return i == 0 ? &p.w1 : i == 1 ? &p.wo : i == 2 ? &p.ws : i == 3 ? &p.w2T : &p.w1T;
    }
    if (k == "wskip") return &c->wskip;
    if (k == "wh1") return &c->wh1;
    if (k == "wh2") return &c->wh2;
    if (k == "wh2T") return &c->wh2T;
    if (k == "wh1T") return &c->wh1T;
    if (k == "wcT") return &c->wcT;
    return nullptr;
}
extern "C" int wn_test_pack_info(wn_ctx* c, const char* kind, int32_t layer, int32_t out[4]) {
    if (!c || !kind || !out) return WN_E_ARG;
    bool per_layer;
    const PackedW* w = find_pack(c, kind, layer, &per_layer);
    if (!w) WN_FAIL(c, WN_E_ARG, "wn_test_pack_info: %s '%s' (layer %d)", per_layer ? "bad layer of pack" : "unknown pack", kind, layer);
    if (!c->packed) WN_FAIL(c, WN_E_STATE, "wn_test_pack_info: wn_pack_weights has not run yet");
    out[0] = w->M; out[1] = w->K; out[2] = w->kil; out[3] = w->gate_interleave;
    return WN_OK;
}
extern "C" int wn_test_pack_copy(wn_ctx* c, const char* kind, int32_t layer, float* out, int64_t n) {
    if (!c || !kind || !out) return WN_E_ARG;
    bool per_layer;
    const PackedW* w = find_pack(c, kind, layer, &per_layer);
    if (!w) WN_FAIL(c, WN_E_ARG, "wn_test_pack_copy: %s '%s' (layer %d)", per_layer ? "bad layer of pack" : "unknown pack", kind, layer);
    const int64_t len = (int64_t)w->M * w->K;
    if (n < len) WN_FAIL(c, WN_E_ARG, "wn_test_pack_copy('%s'): out holds %lld floats, the pack has %lld", kind, (long long)n, (long long)len);
    if (!c->packed) WN_FAIL(c, WN_E_STATE, "wn_test_pack_copy: wn_pack_weights has not run yet");
    WN_HIP(c, hipDeviceSynchronize());          // (the pack launch may still run on the caller's stream)
    hipLaunchKernelGGL(wn_bf16_to_f32, dim3(cdiv(len, 256)), dim3(256), 0, (hipStream_t)0, w->dev.get(), out, len);
    WN_LAUNCH_CHECK(c);
    WN_HIP(c, hipDeviceSynchronize());
    return WN_OK;
}

// ---- test hook: host evaluation of the dropout mask (same inline functions as the kernels)
extern "C" int wn_test_dropout_mask(uint64_t seed, int32_t layer, float p, int64_t first, int64_t n, uint8_t* out) {
    if (!out || n < 0 || first < 0 || !(p >= 0.0f && p < 1.0f)) return WN_E_ARG;
    uint32_t lo, hi; wn_layer_key(seed, layer, &lo, &hi);
    const uint32_t thresh16 = (uint32_t)lrintf(p * 65536.0f);
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t e = (uint32_t)(first + i);
        const uint32_t w = wn_drop_word(lo, hi, e >> 1);
        const uint32_t bits = (e & 1u) ? (w >> 16) : (w & 0xffffu);
        out[i] = bits >= thresh16 ? 1 : 0;
    }
    return WN_OK;
}


// ---- streaming synthesis ------------------------------------------------------------------------------------------------------
extern "C" int wn_synth_stream_lookahead(const wn_config* cfg, int32_t* frames_left, int32_t* frames_right) {
    if (!cfg || !frames_left || !frames_right || cfg->n_upsample < 0 || cfg->n_upsample > WN_MAX_UPSAMPLE) return WN_E_ARG;
    int64_t hop = 1;
    for (int i = 0; i < cfg->n_upsample; ++i) { if (cfg->upsample_scales[i] <= 0) return WN_E_ARG; hop *= cfg->upsample_scales[i]; }
    int32_t l = 0, r = 0;
    if (cfg->upsample_type == WN_UP_SUBPIXEL) {
        // modules.py:578-640: every layer convolves its INPUT with a 3-tap time kernel (SAME) before the shuffle: one input sample of layer i on
        // each side = prod(scales[i:]) samples at the final rate.  [5, 5, 11]: 275 + 55 + 11 = 341 samples = 2 frames; [11, 25]: 2 frames
        int64_t h = 0, later = 1;
        for (int i = cfg->n_upsample - 1; i >= 0; --i) { later *= cfg->upsample_scales[i]; h += later; }
        l = r = (int32_t)((h + hop - 1) / hop);
    } else if (cfg->upsample_type == WN_UP_RESIZE) {
        // modules.py:657-695: nearest resize x s, then an s-tap time kernel (SAME: p = (s-1)/2 before, s-1-p after) at the OUTPUT rate of the layer;
        // p samples of layer i are p * prod(later scales) samples at the final rate.  sum_i < hop / 2: at most one frame on each side
        int64_t hl = 0, hr = 0, later = 1;
        for (int i = cfg->n_upsample - 1; i >= 0; --i) {
            const int s = cfg->upsample_scales[i], p = (s - 1) / 2;
            hl += (int64_t)p * later; hr += (int64_t)(s - 1 - p) * later; later *= s;
        }
        l = (int32_t)((hl + hop - 1) / hop); r = (int32_t)((hr + hop - 1) / hop);
    } else if (cfg->upsample_type != WN_UP_NEAREST && cfg->upsample_type != WN_UP_2D && cfg->upsample_type != WN_UP_1D) return WN_E_ARG;
    *frames_left = l; *frames_right = r;
    return WN_OK;
}

// pending mel frames of the stream: [B][C][w] taken from the previous window (columns drop .. drop + keep) and the pushed frames [B][C][Tn]
__global__ void wn_stream_window_kernel(const float* __restrict__ prev, int64_t prev_cols, int64_t drop, int64_t keep, const float* __restrict__ cnew, int Tn,
                                        float* __restrict__ win, int64_t w, int64_t rows) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * w) return;
    const int64_t row = i / w, col = i - row * w;
    win[i] = col < keep ? prev[row * prev_cols + drop + col] : cnew[row * Tn + (col - keep)];
}

// What a push of `frames` mel frames does to an utterance: frames pushed after it, the frame generation stops at (everything when final, else what the
// right lookahead lets out), samples n it generates, and the window [wstart, pushed) of w frames its conditioning is upsampled from (the left context
// + the frames not yet generated).  `who` names the entry (and slot) in the messages; a rejected push leaves the utterance as it was.
struct WnPushPlan { int64_t pushed, gen_end, n, wstart, w; };
static int plan_push(wn_ctx* c, const char* who, const WnUtt& u, int frames, bool final, int left, int right, WnPushPlan& p) {
    p.pushed = u.pushed + frames;
    p.gen_end = final ? p.pushed : std::max(u.done, p.pushed - right);
    p.n = (p.gen_end - u.done) * c->hop;
    p.wstart = std::max<int64_t>(0, u.done - left); p.w = p.pushed - p.wstart;
    if (p.n > c->maxT) WN_FAIL(c, WN_E_SHAPE, "%s: %lld samples in one push exceed max_time = %d", who, (long long)p.n, c->maxT);
    if (u.done * c->hop + p.n > INT32_MAX) WN_FAIL(c, WN_E_SHAPE, "%s: utterance longer than 2^31 samples", who);
    return WN_OK;
}
static void commit_push(WnUtt& u, const WnPushPlan& p, bool rebuilt) {
    if (rebuilt) { u.cur ^= 1; u.pend_first = p.wstart; }
    u.pushed = p.pushed; u.done = p.gen_end;
}

// stream state buffers, sized for (max_batch, max_time): the window of pending frames never holds more than max_batch x max_time / hop
// frame columns (push checks it), the bias [L][B][G], the carried inputs
static int stream_alloc(wn_ctx* c) {
    auto& S = c->strm;
    for (auto& q : S.pend) WN_HIP(c, q.reserve((size_t)c->C * (c->NT / c->hop + 1)));
    WN_HIP(c, S.carry.reserve(32));
    if (c->gin > 0) WN_HIP(c, S.gbias.reserve((size_t)c->L * std::min(32, c->maxB) * c->G));      // (a stream has at most 32 streams)
    return WN_OK;
}

extern "C" int wn_synth_stream_begin(wn_ctx* c, int32_t B, uint64_t seed, int32_t steps_per_graph, void* stream) {
    if (!c) return WN_E_ARG;
    WnRange range("wn_synth_stream_begin");
    auto& S = c->strm;
    S.open = false; c->slots.open = false;            // (a stream and a slot session exclude one another)
    if (!c->packed) WN_FAIL(c, WN_E_STATE, "wn_pack_weights must be called before wn_synth_stream_begin");
    if (B <= 0 || B > 32 || B > c->maxB) WN_FAIL(c, WN_E_SHAPE, "stream batch %d outside (0, min(32, max_batch = %d)]", B, c->maxB);
    if (c->gin > 0 && (!c->have_g || c->gB != B))
        WN_FAIL(c, WN_E_STATE, "global conditioning is enabled: call wn_set_global_condition with this batch (B=%d) first [wavenet.py:766-777]", B);
    int rc = wn_pipe_check(c, false);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    // the path of wn_synthesize(steps_per_graph) for B (wn_synth_impl), kept for the life of the stream
    const int path = c->cfg.compute_dtype == WN_COMPUTE_F32 ? 3 : wn_synth_takes_pipe(c, B, steps_per_graph) ? 2 : 1;
    if ((rc = wn_noise_reserve(c, B, c->maxT))) return rc;
    if ((rc = path == 3 ? wn_synth_f32_reserve(c, B) : path == 2 ? wn_pipe_reserve(c, B, c->maxT) : wn_synth_reserve(c))) return rc;
    if ((rc = stream_alloc(c))) return rc;
    if (c->gin > 0) {      // the stream's own copy: a training step between pushes rewrites c->gbias
        if ((rc = wn_gbias_fwd(c, B, st))) return rc;
        WN_HIP(c, hipMemcpyAsync(S.gbias, c->gbias, (size_t)c->L * B * c->G * 4, hipMemcpyDeviceToDevice, st));
    }
    wn_synth_stream_lookahead(&c->cfg, &S.left, &S.right);
    S.B = B; S.seed = seed; S.spg = steps_per_graph; S.path = path;
    S.u = WnUtt(); S.poisoned = false;
    S.open = true;
    return WN_OK;
}

extern "C" int wn_synth_stream_push(wn_ctx* c, const float* cc, int32_t Tn, int32_t final, const float* noise, const void* test_inputs,
                                    void* out_samples, float* out_raw, int32_t* n_out, void* stream) {
    if (!c) return WN_E_ARG;
    WnRange range("wn_synth_stream_push");
    auto& S = c->strm;
    if (!S.open) WN_FAIL(c, WN_E_STATE, "wn_synth_stream_push: no open stream (never begun, closed by a final push, or ended by wn_synthesize / "
                                       "wn_pack_weights / wn_set_global_condition / wn_synth_pipe_dtype)");
    if (S.poisoned) WN_FAIL(c, WN_E_STATE, "wn_synth_stream_push: a pipeline run of this stream failed (wn_synth_check); begin a new stream");
    if (Tn < 0 || (Tn > 0 && !cc) || !n_out) WN_FAIL(c, WN_E_ARG, "wn_synth_stream_push: bad frames (Tn = %d) or null n_out", Tn);
    int rc = wn_pipe_check(c, false);                  // a failed earlier push surfaces here at the latest (and poisons the stream)
    if (rc) return rc;
    const int B = S.B, hop = c->hop;
    WnUtt& u = S.u; WnPushPlan pl;
    if ((rc = plan_push(c, "wn_synth_stream_push", u, Tn, final != 0, S.left, S.right, pl))) return rc;
    const int64_t n = pl.n, wstart = pl.wstart, w = pl.w;
    if ((int64_t)B * w * hop > c->NT)
        WN_FAIL(c, WN_E_SHAPE, "wn_synth_stream_push: a window of %lld frames (%d of left context + the frames not yet generated) x %d streams exceeds the workspace", (long long)w, S.left, B);
    if (n > 0 && !out_samples) WN_FAIL(c, WN_E_ARG, "wn_synth_stream_push: null out_samples");
    hipStream_t st = (hipStream_t)stream;
    // pending frames [wstart, pushed): the part of the previous window still needed + the new frames, into the other buffer (the stream's
    // state advances only once everything below is enqueued; a failure after the first enqueue poisons the stream)
    float* win = S.pend[u.cur ^ 1];
    S.poisoned = true;
    if (w > 0) {
        const int64_t rows = (int64_t)B * c->C;
        hipLaunchKernelGGL(wn_stream_window_kernel, dim3(cdiv(rows * w, 256)), dim3(256), 0, st, S.pend[u.cur], u.pushed - u.pend_first, wstart - u.pend_first,
                           u.pushed - wstart, cc, Tn, win, w, rows);
        WN_LAUNCH_CHECK(c);
    }
    if (n > 0) {
        const int T = (int)n;
        // the window's upsampled conditioning (wavenet.py:781-803); rows of the frames generated here are exact: the lookahead keeps every row an
        // artificial window edge touches out of the span (and a window edge at frame 0 / the final frame is the utterance's own edge)
        if ((rc = wn_upsample_fwd(c, nullptr, win, B, (int)w, st))) return rc;
        const int nps = wn_noise_per_step(c);
        if (!noise) {      // the device stream of `seed` over the whole utterance, continued: elements [t0 B nps, (t0 + n) B nps), tempered by the context's pair as it is NOW
            if ((rc = wn_fill_noise_span(c, c->noise_buf, u.done * hop * B * nps, (int64_t)T * B * nps, S.seed, c->tau_scale, c->tau_select, st))) return rc;
            noise = c->noise_buf;
        } else if (c->tau_scale != 1.0f || c->tau_select != 1.0f) {      // the run reads a tempered copy (T <= max_time: reserved at wn_synth_stream_begin); the caller's buffer is not written
            if ((rc = wn_temper_noise_impl(c, noise, c->noise_buf, B, T, c->tau_scale, c->tau_select, st))) return rc;
            noise = c->noise_buf;
        }
        WnSpan sp;
        sp.t0 = (int)(u.done * hop); sp.Tcb = (int)(w * hop); sp.cbt_off = (int)((u.done - wstart) * hop); sp.carry = S.carry; sp.gbias = S.gbias;
        rc = S.path == 2 ? wn_pipe_span(c, B, T, sp, noise, test_inputs, out_samples, out_raw, st)
           : S.path == 3 ? wn_synth_f32_span(c, B, T, sp, noise, test_inputs, out_samples, out_raw, S.spg, st)
                         : wn_synth_span(c, B, T, sp, noise, test_inputs, out_samples, out_raw, S.spg, st);
        if (rc) return rc;
        c->fB = B; c->fT = T; c->fTc = (int)(pl.gen_end - u.done); c->fup_off = sp.cbt_off; c->fup_pitch = sp.Tcb;
    }
    S.poisoned = false;
    commit_push(u, pl, true);
    *n_out = (int32_t)n;
    if (final) S.open = false;
    return WN_OK;
}

extern "C" int wn_synth_stream_end(wn_ctx* c) {
    if (!c) return WN_E_ARG;
    c->strm.open = false;
    return WN_OK;
}

// ---- synthesis slots: utterances join and leave a running batch -------------------------------------------------------------------
// One session = B slots on one path / pipeline configuration.  What a stream keeps once (time index, pending window, seed, carried input, bias row) a
// session keeps per slot; a push runs max_b n_out[b] steps in which every slot takes part, the ones that have nothing (more) to generate as dummies.
// the host arrays of one push, one entry per slot (st0 / snl padded to whole tiles); sized with the tables, so that a push allocates nothing
struct wn_ctx::WnSlots::PushHost {
    std::vector<WnPushPlan> pl; std::vector<int64_t> w, first, cnt; std::vector<int> nb; std::vector<uint8_t> rebuilt, grouped; std::vector<float> ts, tsel;
    std::vector<uint64_t> seed; std::vector<int32_t> st0, snl; std::vector<uint32_t> fresh;
    explicit PushHost(int n) : pl(n), w(n), first(n), cnt(n), nb(n), rebuilt(n), grouped(n), ts(n), tsel(n), seed(n), st0(32 * ((n + 31) / 32)), snl(st0.size()), fresh(st0.size() / 32) {}
};
int wn_slots_alloc(wn_ctx* c, int nslots) {
    auto& S = c->slots;
    int l = 0, r = 0; wn_synth_stream_lookahead(&c->cfg, &l, &r);
    S.capw = c->maxT / c->hop + l + r + 1;
    nslots = std::max(nslots, std::min(32, c->maxB));      // (never fewer than a narrow session may ask for: its begin does not grow them)
    if (nslots > S.cap_slots) {      // the tables that hold one entry or region per slot (a training context grows them at begin; inference-only: sized once, at wn_create)
        if (c->inference && S.cap_slots > 0) WN_FAIL(c, WN_E_SHAPE, "slot session: %d slots exceed the %d this inference-only context was sized for", nslots, S.cap_slots);
        if (S.cap_slots > 0) WN_HIP(c, hipDeviceSynchronize());      // (growing: nothing may still read the old tables)
        const int nb = std::min(32, nslots);
        for (auto& q : S.pend) WN_HIP(c, q.grow((size_t)nslots * c->C * S.capw));
        WN_HIP(c, S.gwin.grow((size_t)nb * c->C * S.capw));      // (a conditioning group has at most 32 members)
        WN_HIP(c, S.tdev.grow((size_t)((nslots + 31) / 32) * WN_SL_STRIDE));
        if (c->gin > 0) WN_HIP(c, S.gbias.grow((size_t)c->L * nslots * c->G));
        S.s.assign(nslots, wn_ctx::WnSlots::Slot());
        S.ph = std::make_shared<wn_ctx::WnSlots::PushHost>(nslots);
        S.cap_slots = nslots;
    }
    WN_HIP(c, S.cbt.reserve((size_t)c->NT * c->C));
    WN_HIP(c, S.feat.reserve((size_t)c->NT * c->C));
    WN_HIP(c, S.carry.reserve(32));
    // folded synthesis: whole utterances of up to max_batch x max_time samples in all, the rows' samples / teacher-forcing inputs, the fade tables
    WN_HIP(c, S.fwin.reserve((size_t)c->C * (c->NT / c->hop + 1)));
    WN_HIP(c, S.frow.reserve((size_t)c->NT));
    WN_HIP(c, S.fti.reserve((size_t)c->NT));
    WN_HIP(c, S.fw.reserve((size_t)2 * c->NT));
    return WN_OK;
}

// both begins: `wide` opens the session on the wide owner of the launch-per-layer path (any B <= max_batch), else on the path of wn_synthesize(steps_per_graph) for B <= 32
static int slots_begin(wn_ctx* c, const char* who, int B, int steps_per_graph, hipStream_t st, bool wide) {
    auto& S = c->slots;
    S.open = false; c->strm.open = false;                 // a slot session and a stream exclude one another; one session at a time, narrow or wide
    if (c->cfg.compute_dtype == WN_COMPUTE_F32) WN_FAIL(c, WN_E_UNSUPPORTED, "%s: slot sessions are not built for the fp32 validation mode (compute_dtype = WN_COMPUTE_F32)", who);
    if (!c->packed) WN_FAIL(c, WN_E_STATE, "wn_pack_weights must be called before %s", who);
    if (wide) { if (B <= 0 || B > c->maxB) WN_FAIL(c, WN_E_SHAPE, "wide slot count %d outside (0, max_batch = %d]", B, c->maxB); }
    else if (B <= 0 || B > 32 || B > c->maxB) WN_FAIL(c, WN_E_SHAPE, "slot count %d outside (0, min(32, max_batch = %d)]", B, c->maxB);
    int rc = wn_pipe_check(c, false);
    if (rc) return rc;
    const int path = !wide && wn_synth_takes_pipe(c, B, steps_per_graph) ? 2 : 1;
    if ((rc = wn_noise_reserve(c, B, c->maxT))) return rc;
    if ((rc = wide ? wn_synth_wide_reserve(c, B) : path == 2 ? wn_pipe_reserve(c, B, c->maxT) : wn_synth_reserve(c))) return rc;
    if ((rc = wn_slots_alloc(c, B))) return rc;
    wn_synth_stream_lookahead(&c->cfg, &S.left, &S.right);
    WN_HIP(c, hipMemsetAsync(S.tdev, 0, (size_t)((B + 31) / 32) * WN_SL_STRIDE * 4, st));
    S.B = B; S.spg = steps_per_graph; S.path = path; S.wide = wide; S.poisoned = false; S.first_run = true;
    for (auto& s : S.s) s = wn_ctx::WnSlots::Slot();
    S.open = true;
    return WN_OK;
}
extern "C" int wn_synth_slots_begin(wn_ctx* c, int32_t B, int32_t steps_per_graph, void* stream) {
    if (!c) return WN_E_ARG;
    WnRange range("wn_synth_slots_begin");
    return slots_begin(c, "wn_synth_slots_begin", B, steps_per_graph, (hipStream_t)stream, false);
}
// The same session for any 0 < B <= max_batch, always on the launch-per-layer path: ceil(B / 32) tiles of slots per launch on the wide owner (wn_synth.hip)
extern "C" int wn_synth_wide_slots_begin(wn_ctx* c, int32_t B, int32_t steps_per_graph, void* stream) {
    if (!c) return WN_E_ARG;
    WnRange range("wn_synth_wide_slots_begin");
    return slots_begin(c, "wn_synth_wide_slots_begin", B, steps_per_graph, (hipStream_t)stream, true);
}

static int slots_usable(wn_ctx* c, const char* who) {
    auto& S = c->slots;
    if (!S.open) WN_FAIL(c, WN_E_STATE, "%s: no open slot session (never begun, or ended by wn_synthesize / wn_pack_weights / wn_synth_pipe_dtype / wn_synth_stream_begin)", who);
    if (S.poisoned) WN_FAIL(c, WN_E_STATE, "%s: a pipeline run of this session failed (wn_synth_check); begin a new session", who);
    return WN_OK;
}

extern "C" int wn_synth_slot_open(wn_ctx* c, int32_t slot, uint64_t seed, const void* g, void* stream) {
    if (!c) return WN_E_ARG;
    int rc = slots_usable(c, "wn_synth_slot_open");
    if (rc) return rc;
    auto& S = c->slots;
    if (slot < 0 || slot >= S.B) WN_FAIL(c, WN_E_ARG, "wn_synth_slot_open: slot %d outside [0, %d)", slot, S.B);
    if ((c->gin > 0) != (g != nullptr)) WN_FAIL(c, WN_E_ARG, "wn_synth_slot_open: g must be given iff the model has global conditioning (gin_channels = %d)", c->gin);
    if (S.s[slot].live) WN_FAIL(c, WN_E_STATE, "wn_synth_slot_open: slot %d carries an utterance (finish it with a final push or wn_synth_slot_abandon)", slot);
    if (c->gin > 0 && (rc = wn_gbias_row(c, g, S.gbias, S.B, slot, (hipStream_t)stream))) return rc;
    auto& s = S.s[slot];
    s = wn_ctx::WnSlots::Slot(); s.live = true; s.seed = seed; s.tau_scale = c->tau_scale; s.tau_select = c->tau_select;
    return WN_OK;
}

extern "C" int wn_synth_set_slot_temperature(wn_ctx* c, int32_t slot, float tau_scale, float tau_select) {
    if (!c) return WN_E_ARG;
    int rc = slots_usable(c, "wn_synth_set_slot_temperature");
    if (rc) return rc;
    auto& S = c->slots;
    if (slot < 0 || slot >= S.B) WN_FAIL(c, WN_E_ARG, "wn_synth_set_slot_temperature: slot %d outside [0, %d)", slot, S.B);
    if ((rc = tau_check(c, "wn_synth_set_slot_temperature", tau_scale, tau_select))) return rc;
    if (!S.s[slot].live) WN_FAIL(c, WN_E_STATE, "wn_synth_set_slot_temperature: slot %d is idle (wn_synth_slot_open first)", slot);
    S.s[slot].tau_scale = tau_scale; S.s[slot].tau_select = tau_select;      // host state: from the next push on
    return WN_OK;
}

extern "C" int wn_synth_slot_abandon(wn_ctx* c, int32_t slot) {
    if (!c) return WN_E_ARG;
    int rc = slots_usable(c, "wn_synth_slot_abandon");
    if (rc) return rc;
    if (slot < 0 || slot >= c->slots.B) WN_FAIL(c, WN_E_ARG, "wn_synth_slot_abandon: slot %d outside [0, %d)", slot, c->slots.B);
    c->slots.s[slot].live = false;
    return WN_OK;
}

extern "C" int wn_synth_slot_frames_done(const wn_ctx* c, int32_t slot) {
    if (!c) return WN_E_ARG;
    if (!c->slots.open || c->slots.poisoned) return WN_E_STATE;
    if (slot < 0 || slot >= c->slots.B) return WN_E_ARG;
    return c->slots.s[slot].live ? (int)c->slots.s[slot].u.done : -1;
}

extern "C" int wn_synth_slots_end(wn_ctx* c) {
    if (!c) return WN_E_ARG;
    c->slots.open = false;
    return WN_OK;
}

// every rebuilt slot's pending window of a tile of 32 slots (b0 + blockIdx.y) in ONE launch: [C][w] dense = the kept columns of its previous window + its
// leading frames of the pushed block
struct WnSlotWin { int32_t prev_cols[32], drop[32], keep[32], w[32], cur[32]; };
__global__ void wn_slots_window_kernel(const float* __restrict__ p0, const float* __restrict__ p1, float* __restrict__ q0, float* __restrict__ q1, int64_t region,
                                       const float* __restrict__ cnew, int Tn, int C, WnSlotWin p, int b0) {
    const int k = blockIdx.y, w = p.w[k];
    const int64_t b = (int64_t)b0 + k;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w <= 0 || i >= (int64_t)C * w) return;
    const int64_t row = i / w, col = i - row * w;
    const float* prev = (p.cur[k] ? p1 : p0) + region * b;
    float* win = (p.cur[k] ? q0 : q1) + region * b;
    win[i] = col < p.keep[k] ? prev[row * p.prev_cols[k] + p.drop[k] + col] : cnew[(b * C + row) * Tn + (col - p.keep[k])];
}
// the windows of a group of slots side by side [g][C][w] (the upsample net takes a batch of equal width), and back: the rows of every member's span out of
// the group's upsampled conditioning into the session's table cbt [B][n_max][C] (bf16) / feat [B][C][n_max] (fp32).  slot[]: the members' slots of the
// SESSION (any tile), so a group needs no slot base
struct WnSlotGrp { int32_t slot[32], cur[32], off[32], n[32]; };
__global__ void wn_slots_gather_kernel(const float* __restrict__ p0, const float* __restrict__ p1, int64_t region, float* __restrict__ gwin, int64_t cw, WnSlotGrp p) {
    const int g = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cw) return;
    gwin[(int64_t)g * cw + i] = ((p.cur[g] ? p1 : p0) + region * p.slot[g])[i];
}
__global__ void wn_slots_scatter_kernel(const bf16_t* __restrict__ cbt, const float* __restrict__ cup, int64_t Tw, int C, bf16_t* __restrict__ scbt, float* __restrict__ feat,
                                        int64_t n_max, WnSlotGrp p) {
    const int g = blockIdx.y, n = p.n[g], b = p.slot[g];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n * C) return;
    { const int64_t t = i / C, ch = i - t * C; scbt[((int64_t)b * n_max + t) * C + ch] = cbt[((int64_t)g * Tw + p.off[g] + t) * C + ch]; }
    { const int64_t ch = i / n, t = i - ch * n; feat[((int64_t)b * C + ch) * n_max + t] = cup[((int64_t)g * C + ch) * Tw + p.off[g] + t]; }
}

extern "C" int wn_synth_slots_push(wn_ctx* c, const float* cc, int32_t Tn, const int32_t* frames, const int32_t* final_, const float* noise, const void* test_inputs,
                                   void* out_samples, float* out_raw, int32_t out_pitch, int32_t* n_out, void* stream) {
    if (!c) return WN_E_ARG;
    WnRange range("wn_synth_slots_push");
    int rc = slots_usable(c, "wn_synth_slots_push");
    if (rc) return rc;
    auto& S = c->slots;
    if (Tn < 0 || (Tn > 0 && !cc) || !frames || !final_ || !n_out) WN_FAIL(c, WN_E_ARG, "wn_synth_slots_push: bad frames (Tn = %d) or a null host array", Tn);
    if ((rc = wn_pipe_check(c, false))) return rc;       // a failed earlier push surfaces here at the latest (and poisons the session)
    if (S.poisoned) WN_FAIL(c, WN_E_STATE, "wn_synth_slots_push: a pipeline run of this session failed; begin a new session");
    const int B = S.B, hop = c->hop, C = c->C;
    // ---- plan (host only: a rejected push leaves every slot as it was).  The arrays of a push hold one entry per slot and belong to the session.
    auto& H = *S.ph;
    WnPushPlan* const pl = H.pl.data(); int64_t* const w = H.w.data(); int* const nb = H.nb.data(); int n_max = 0;
    for (int b = 0; b < B; ++b) {
        const auto& s = S.s[b];
        nb[b] = 0; w[b] = 0; pl[b] = WnPushPlan();
        if (frames[b] < 0 || frames[b] > Tn) WN_FAIL(c, WN_E_ARG, "wn_synth_slots_push: frames[%d] = %d outside [0, Tn = %d]", b, frames[b], Tn);
        if (!s.live) { if (frames[b] > 0) WN_FAIL(c, WN_E_STATE, "wn_synth_slots_push: %d frames for slot %d, which is idle (wn_synth_slot_open first)", frames[b], b); continue; }
        char who[40]; snprintf(who, sizeof who, "wn_synth_slots_push: slot %d", b);
        if ((rc = plan_push(c, who, s.u, frames[b], final_[b] != 0, S.left, S.right, pl[b]))) return rc;
        w[b] = pl[b].w;
        if (w[b] > S.capw || (pl[b].n > 0 && w[b] * hop > c->NT))
            WN_FAIL(c, WN_E_SHAPE, "%s: a window of %lld frames (%d of left context + the frames not yet generated) exceeds the workspace", who, (long long)w[b], S.left);
        nb[b] = (int)pl[b].n; n_max = std::max(n_max, nb[b]);
    }
    if (n_max > 0 && (!out_samples || out_pitch < n_max)) WN_FAIL(c, WN_E_ARG, "wn_synth_slots_push: null out_samples or out_pitch %d < %d samples", out_pitch, n_max);
    hipStream_t st = (hipStream_t)stream;
    const int64_t region = (int64_t)C * S.capw;
    S.poisoned = true;                                    // (the state advances only once everything is enqueued; a failure after the first enqueue poisons the session)
    // ---- pending windows of the slots that received frames or dropped generated ones
    uint8_t* const rebuilt = H.rebuilt.data();
    for (int b0 = 0; b0 < B; b0 += 32) {      // (the parameters travel by value: one launch per tile of 32 slots that has a window to rebuild)
        const int nbt = std::min(32, B - b0);
        WnSlotWin p; memset(&p, 0, sizeof p); int64_t wmax = 0;
        for (int k = 0; k < nbt; ++k) {
            const int b = b0 + k;
            const WnUtt& u = S.s[b].u; const int64_t wstart = pl[b].wstart;
            rebuilt[b] = 0;
            if (!S.s[b].live || w[b] <= 0 || (frames[b] == 0 && wstart == u.pend_first)) continue;
            p.prev_cols[k] = (int)(u.pushed - u.pend_first); p.drop[k] = (int)(wstart - u.pend_first); p.keep[k] = (int)(u.pushed - wstart); p.w[k] = (int)w[b]; p.cur[k] = u.cur;
            rebuilt[b] = 1; wmax = std::max(wmax, w[b]);
        }
        if (wmax > 0) {
            hipLaunchKernelGGL(wn_slots_window_kernel, dim3(cdiv(C * wmax, 256), nbt), dim3(256), 0, st, S.pend[0], S.pend[1], S.pend[0], S.pend[1], region, cc, Tn, C, p, b0);
            WN_LAUNCH_CHECK(c);
        }
    }
    if (n_max > 0) {
        // ---- conditioning (wavenet.py:781-803): slots of equal window width are upsampled as one batch; every window starts at its utterance's own frame
        // max(0, done - left) and ends at its own last pushed frame, so an edge is either the utterance's own or outside what the lookahead lets a span read
        uint8_t* const grouped = H.grouped.data(); memset(grouped, 0, (size_t)B);
        for (int b0 = 0; b0 < B; ++b0) {
            if (nb[b0] <= 0 || grouped[b0]) continue;
            const int64_t gw = w[b0];
            const int gcap = (int)std::max<int64_t>(1, std::min<int64_t>(32, c->NT / (gw * hop)));
            WnSlotGrp g; memset(&g, 0, sizeof g); int ng = 0; int nmaxg = 0;
            for (int b = b0; b < B && ng < gcap; ++b) {
                if (nb[b] <= 0 || grouped[b] || w[b] != gw) continue;
                grouped[b] = 1;
                g.slot[ng] = b; g.cur[ng] = S.s[b].u.cur ^ (rebuilt[b] ? 1 : 0); g.off[ng] = (int)((S.s[b].u.done - pl[b].wstart) * hop); g.n[ng] = nb[b]; nmaxg = std::max(nmaxg, nb[b]); ++ng;
            }
            hipLaunchKernelGGL(wn_slots_gather_kernel, dim3(cdiv(C * gw, 256), ng), dim3(256), 0, st, S.pend[0], S.pend[1], region, S.gwin, C * gw, g);
            WN_LAUNCH_CHECK(c);
            if ((rc = wn_upsample_fwd(c, nullptr, S.gwin, ng, (int)gw, st))) return rc;
            hipLaunchKernelGGL(wn_slots_scatter_kernel, dim3(cdiv((int64_t)nmaxg * C, 256), ng), dim3(256), 0, st, c->cbt, c->CUP[c->cup_final_idx], gw * hop, C, S.cbt, S.feat,
                               (int64_t)n_max, g);
            WN_LAUNCH_CHECK(c);
        }
        float* const ts = H.ts.data(); float* const tsel = H.tsel.data(); bool tempered = false;      // every slot's own pair; rows of slots that do not generate are ignored
        for (int b = 0; b < B; ++b) { ts[b] = S.s[b].tau_scale; tsel[b] = S.s[b].tau_select; tempered |= nb[b] > 0 && (ts[b] != 1.0f || tsel[b] != 1.0f); }
        if (!noise) {      // every generating slot's own one-stream noise, continued at its sample done * hop
            uint64_t* const seed = H.seed.data(); int64_t* const first = H.first.data(); int64_t* const cnt = H.cnt.data(); const int nps = wn_noise_per_step(c);
            for (int b = 0; b < B; ++b) { seed[b] = S.s[b].seed; first[b] = S.s[b].u.done * hop * nps; cnt[b] = (int64_t)nb[b] * nps; }
            if ((rc = wn_fill_noise_slots(c, c->noise_buf, B, seed, first, cnt, ts, tsel, st))) return rc;
            noise = c->noise_buf;
        } else if (tempered) {      // a tempered copy, column by column (n_max <= max_time: reserved at wn_synth_slots_begin); the caller's buffer is not written
            if ((rc = wn_temper_noise_cols(c, noise, c->noise_buf, B, n_max, ts, tsel, st))) return rc;
            noise = c->noise_buf;
        }
        int32_t* const st0 = H.st0.data(); int32_t* const snl = H.snl.data(); uint32_t* const fresh = H.fresh.data();      // (padded to whole tiles of 32)
        const int Bp = 32 * ((B + 31) / 32);
        for (int k = 0; 32 * k < Bp; ++k) fresh[k] = 0;
        for (int b = 0; b < Bp; ++b) { st0[b] = b < B ? (int)(S.s[b].u.done * hop) : 0; snl[b] = b < B ? nb[b] : 0; if (b < B && nb[b] > 0 && S.s[b].u.done == 0) fresh[b >> 5] |= 1u << (b & 31); }
        WnSpan sp;
        sp.t0 = 0; sp.Tcb = n_max; sp.cbt_off = 0; sp.carry = S.carry; sp.gbias = S.gbias;
        sp.st0 = st0; sp.snl = snl; sp.out_pitch = out_pitch; sp.cbt = S.cbt; sp.reslice = S.first_run; sp.tdev = S.tdev; sp.fresh = fresh;
        rc = S.wide ? wn_synth_wide_span(c, B, n_max, sp, noise, test_inputs, out_samples, out_raw, S.spg, st)
           : S.path == 2 ? wn_pipe_span(c, B, n_max, sp, noise, test_inputs, out_samples, out_raw, st)
                         : wn_synth_span(c, B, n_max, sp, noise, test_inputs, out_samples, out_raw, S.spg, st);
        if (rc) return rc;
        S.first_run = false;
        c->fB = B; c->fT = n_max; c->fTc = 0; c->fup_pitch = -1; S.feat_pitch = n_max; S.feat_B = B;
    }
    S.poisoned = false;
    for (int b = 0; b < B; ++b) {
        auto& s = S.s[b];
        n_out[b] = nb[b];
        if (!s.live) continue;
        commit_push(s.u, pl[b], rebuilt[b]);
        if (final_[b]) s.live = false;
    }
    return WN_OK;
}
