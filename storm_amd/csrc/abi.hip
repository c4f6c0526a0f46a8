// Error channel, version and device info of libstorm_hip.
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "common.h"
#include "tasnet.h"

namespace storm {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

void bump_switch_epoch();
namespace {
struct SwitchName { const char* name; int Switches::*field; };
const SwitchName kSwitches[] = {
    {"STORM_CONV_VARIANT", &Switches::conv_variant}, {"STORM_CONV_PIPE128", &Switches::conv_pipe128}, 
    {"STORM_CONV_CUS", &Switches::conv_cus}, {"STORM_CONV_PERSIST", &Switches::conv_persist},
    {"STORM_CONV_DMA", &Switches::conv_dma}, {"STORM_CONV_ABLATE", &Switches::conv_ablate}, {"STORM_SPLITK", &Switches::splitk}, {"STORM_GN_WIDE", &Switches::gn_wide}, {"STORM_GN_DOWN_SHARE", &Switches::gn_down_share}, {"STORM_GN_ROWS", &Switches::gn_rows}, {"STORM_GN_NT", &Switches::gn_nt}, {"STORM_GRAPH", &Switches::graph}, {"STORM_SPLITK_SMALL", &Switches::splitk_small}, {"STORM_CONV_TABLE", &Switches::conv_table}, {"STORM_ATTN_SPLIT", &Switches::attn_split}, {"STORM_BATCH_INVARIANT", &Switches::batch_invariant}, {"STORM_XCORR_LAGS", &Switches::xcorr_lags}, {"STORM_BSS_LAGS", &Switches::bss_lags},
};
}  // namespace

Switches& switches() {
    static Switches sw = [] {
        Switches v;
        for (const SwitchName& n : kSwitches)
            if (const char* e = getenv(n.name)) v.*(n.field) = atoi(e);
        if (const char* e = getenv("STORM_CONV_TRACE_PTR")) v.conv_trace_ptr = strtoull(e, nullptr, 0);
        return v;
    }();
    return sw;
}

static std::atomic<unsigned long long> g_switch_epoch{0};
unsigned long long switch_epoch() { return g_switch_epoch.load(std::memory_order_relaxed); }
void bump_switch_epoch() { g_switch_epoch.fetch_add(1, std::memory_order_relaxed); }

int device_cus() {
    const int forced = switches().conv_cus;
    if (forced > 0) return forced;
    static int n_cu = 0;
    if (n_cu == 0) {
        int dev = 0; hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n_cu = prop.multiProcessorCount;
        if (n_cu <= 0) n_cu = 256;
    }
    return n_cu;
}
}  // namespace storm

// Test / tool hook (not part of the drop-in surface): set one of the switches above by its environment-variable name.
extern "C" int storm_set_switch(const char* name, long long value) {
    STORM_CHECK(name != nullptr, "storm_set_switch: null name");
    if (strcmp(name, "STORM_CONV_TRACE_PTR") == 0) { storm::switches().conv_trace_ptr = (unsigned long long)value; return STORM_OK; }
    for (const storm::SwitchName& n : storm::kSwitches)
        if (strcmp(name, n.name) == 0) { storm::switches().*(n.field) = (int)value; storm::bump_switch_epoch(); return STORM_OK; }
    STORM_CHECK(false, "storm_set_switch: unknown switch %s", name);
}
extern "C" long long storm_get_switch(const char* name) {
    if (name == nullptr) return 0;
    if (strcmp(name, "STORM_CONV_TRACE_PTR") == 0) return (long long)storm::switches().conv_trace_ptr;
    for (const storm::SwitchName& n : storm::kSwitches)
        if (strcmp(name, n.name) == 0) return storm::switches().*(n.field);
    return 0;
}

extern "C" const char* storm_last_error(void) { return storm::g_err; }
extern "C" int storm_abi_version(void) { return STORM_ABI_VERSION; }
extern "C" long long storm_abi_struct_bytes(int which) {
    switch (which) {
        case 0: return (long long)sizeof(storm_conv_args);
        case 1: return (long long)sizeof(storm_op);
        case 2: return (long long)sizeof(storm_conv_seg);
        case 3: return (long long)sizeof(storm_ncsnpp_config);
        case 4: return (long long)sizeof(storm_ncsnpp_config_ex);
        default: return -1;
    }
}
extern "C" int storm_device_info(char* name, int name_len, int* n_cu, size_t* hbm_bytes) {
    int dev = 0;
    STORM_HIP(hipGetDevice(&dev));
    hipDeviceProp_t p;
    STORM_HIP(hipGetDeviceProperties(&p, dev));
    if (name && name_len > 0) { strncpy(name, p.gcnArchName, name_len - 1); name[name_len - 1] = 0; }
    if (n_cu) *n_cu = p.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = p.totalGlobalMem;
    return STORM_OK;
}

// ---- ConvTasNet op-level entry points (kernels: tasnet.h, compiled with spectral.hip) ----
static bool tasnet_dtype_ok(int dtype) { return dtype == STORM_F32 || dtype == STORM_BF16 || dtype == STORM_F16; }
extern "C" int storm_tasnet_num_partials(int op, int L, int C) {
    if (op < STORM_TASNET_ENCODE || op > STORM_TASNET_DEPTHWISE || L <= 0 || C <= 0 || C % 8) return -1;
    return storm::tasnet_num_partials(op, L, C);
}
extern "C" int storm_tasnet_frames(long long T, int win) {
    const int stride = win / 2;
    if (T <= 0 || win < 2 || T > (1ll << 40)) return -1;
    const long long rest = win - (stride + T % win) % win;                  // convtasnet.py:86
    const long long frames = (T + rest + 2 * stride - win) / stride + 1;
    return frames > 0x7fffffffll / 2 ? -1 : (int)frames;
}
extern "C" int storm_tasnet_encode(const float* wav, long long wav_stride, const float* wT, void* enc, float* part, int B, long long T,
                                   int N, int win, int dtype, storm_stream_t s) {
    STORM_CHECK(wav && wT && enc && part, "storm_tasnet_encode: null pointer");
    STORM_CHECK(B > 0 && B <= 65535 && T > 0 && wav_stride >= T && win >= 2 && N > 0 && N % 8 == 0 && tasnet_dtype_ok(dtype),
                "storm_tasnet_encode: B=%d T=%lld stride=%lld N=%d win=%d dtype=%d", B, T, wav_stride, N, win, dtype);
    const int L = storm_tasnet_frames(T, win);
    STORM_CHECK(L > 0 && (long long)L * N < (1ll << 40), "storm_tasnet_encode: %lld samples do not frame", T);
    return storm::launch_tasnet_encode(wav, wav_stride, wT, enc, part, B, T, N, win, win / 2, L, dtype, (hipStream_t)s);
}
extern "C" int storm_tasnet_gln_finalize(const float* part, float* stats, int B, int nparts, long long count, float eps, storm_stream_t s) {
    STORM_CHECK(part && stats && B > 0 && nparts > 0 && count > 0 && eps >= 0.f, "storm_tasnet_gln_finalize: bad arguments");
    return storm::launch_tasnet_gln_finalize(part, stats, B, nparts, count, eps, (hipStream_t)s);
}
extern "C" int storm_tasnet_pointwise(const void* x, int x_f32, const void* w, const float* bias, void* out, int out_f32, float* skip,
                                      int res_skip, const float* norm_stats, const float* gamma, const float* beta, const float* prelu_in,
                                      const float* prelu_out, float* part, int B, int L, int Cin, int Cout, int dtype, storm_stream_t s) {
    STORM_CHECK(x && w && bias && out, "storm_tasnet_pointwise: null pointer");
    STORM_CHECK(B > 0 && B <= 65535 && L > 0 && Cin > 0 && Cout > 0 && Cin % 8 == 0 && Cout % 8 == 0 && tasnet_dtype_ok(dtype),
                "storm_tasnet_pointwise: B=%d L=%d Cin=%d Cout=%d dtype=%d (channel counts are multiples of 8)", B, L, Cin, Cout, dtype);
    STORM_CHECK(!norm_stats || (gamma && beta), "storm_tasnet_pointwise: norm-on-load needs gamma and beta");
    STORM_CHECK(!(norm_stats && prelu_in), "storm_tasnet_pointwise: norm-on-load and PReLU-on-load exclude each other");
    STORM_CHECK(!res_skip || (skip && Cout % 16 == 0 && !prelu_out && !part), "storm_tasnet_pointwise: res_skip needs skip, Cout = 2 BN with BN %% 8 == 0, and has no PReLU / partials");
    STORM_CHECK((storm::cdiv(Cout, storm::TASNET_PW_COLS)) <= 65535, "storm_tasnet_pointwise: Cout=%d", Cout);
    storm::TasnetPointwise p{x, w, bias, out, skip, norm_stats, gamma, beta, prelu_in, prelu_out, part, L, Cin, Cout,
                             (x_f32 && dtype != STORM_F32) ? 1 : 0, out_f32 ? 1 : 0, res_skip ? 1 : 0};
    return storm::launch_tasnet_pointwise(p, B, dtype, (hipStream_t)s);
}
extern "C" int storm_tasnet_depthwise(const void* x, const float* w3, const float* bias, const float* norm_stats, const float* gamma,
                                      const float* beta, const float* prelu, void* out, float* part, int B, int L, int C, int dilation,
                                      int dtype, storm_stream_t s) {
    STORM_CHECK(x && w3 && bias && norm_stats && gamma && beta && prelu && out && part, "storm_tasnet_depthwise: null pointer");
    STORM_CHECK(B > 0 && B <= 65535 && L > 0 && C > 0 && C % 8 == 0 && dilation >= 1 && tasnet_dtype_ok(dtype) && x != out,
                "storm_tasnet_depthwise: B=%d L=%d C=%d dilation=%d dtype=%d", B, L, C, dilation, dtype);
    return storm::launch_tasnet_depthwise(x, w3, bias, norm_stats, gamma, beta, prelu, out, part, B, L, C, dilation, dtype, (hipStream_t)s);
}
extern "C" int storm_tasnet_decode(const void* mask, const void* enc, const float* wd, float* out, int B, int L, int N, int win, int dtype,
                                   storm_stream_t s) {
    STORM_CHECK(mask && enc && wd && out, "storm_tasnet_decode: null pointer");
    STORM_CHECK(B > 0 && B <= 65535 && L > 0 && N > 0 && N % 8 == 0 && win >= 2 && tasnet_dtype_ok(dtype),
                "storm_tasnet_decode: B=%d L=%d N=%d win=%d dtype=%d", B, L, N, win, dtype);
    return storm::launch_tasnet_decode(mask, enc, wd, out, B, L, N, win, win / 2, dtype, (hipStream_t)s);
}
