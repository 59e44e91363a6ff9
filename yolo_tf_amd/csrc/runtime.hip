// Pieces of the C ABI that belong to no kernel family: error string, deterministic flag, CRC32C, ABI version, the debug entries.
#include "common.h"
#include <stdarg.h>

// ------------------------------------------------------------------------------------------
// error string (thread local) + misc ABI
// ------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void yolo2_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char *yolo2_last_error(void) { return g_err; }

// deterministic mode of the CALLING THREAD (include/yolo2_hip.h yolo2_set_deterministic): launch rules and reductions that would sum floats in arrival
// order take a fixed-order form instead.  Thread-local like the error string; a deterministic engine switches it on for the duration of its own sweeps only.
static thread_local int g_deterministic = 0;
int y2_deterministic() { return g_deterministic; }
extern "C" int yolo2_set_deterministic(int on) { g_deterministic = on ? 1 : 0; return YOLO2_OK; }
extern "C" int yolo2_get_deterministic(void) { return g_deterministic; }

int y2_device_cus() {
    static const int cus = [] {
        hipDeviceProp_t prop;
        int dev = 0;
        return (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    }();
    return cus;
}

// CRC32C (Castagnoli) of a HOST buffer, slicing-by-8: the checksum of TFRecord / TensorBoard event / TF checkpoint files
// (utils/tfrecord.py, utils/events.py, tf_checkpoint.py); `crc` = value so far (0 to start).  ~1.5 GB/s, against ~1 MB/s in Python.
extern "C" uint32_t yolo2_crc32c(const void *data, size_t n, uint32_t crc) {
    static uint32_t table[8][256];
    static bool ready = [] {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
            table[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int t = 1; t < 8; ++t) table[t][i] = (table[t - 1][i] >> 8) ^ table[0][table[t - 1][i] & 0xFF];
        return true;
    }();
    (void)ready;
    const unsigned char *p = (const unsigned char *)data;
    crc = ~crc;
    while (n && ((uintptr_t)p & 7)) { crc = table[0][(crc ^ *p++) & 0xFF] ^ (crc >> 8); --n; }
    while (n >= 8) {
        uint64_t w;
        __builtin_memcpy(&w, p, 8);
        w ^= crc;
        crc = table[7][w & 0xFF] ^ table[6][(w >> 8) & 0xFF] ^ table[5][(w >> 16) & 0xFF] ^ table[4][(w >> 24) & 0xFF] ^
              table[3][(w >> 32) & 0xFF] ^ table[2][(w >> 40) & 0xFF] ^ table[1][(w >> 48) & 0xFF] ^ table[0][(w >> 56) & 0xFF];
        p += 8;
        n -= 8;
    }
    while (n--) crc = table[0][(crc ^ *p++) & 0xFF] ^ (crc >> 8);
    return ~crc;
}
extern "C" int yolo2_abi_version(void) { return 1; }

// empty kernel: bench.py calibrates what a HIP-event bracket adds to the kernel it brackets (dispatch latency between the start
// event's completion and the kernel's first wave) by bracketing this
__global__ void noop_kernel() {}
extern "C" int yolo2_debug_noop(void *stream) {
    noop_kernel<<<1, 64, 0, (hipStream_t)stream>>>();
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

// ------------------------------------------------------------------------------------------
// layout self-test for ds_read_b64_tr_b16 (used once on hardware to confirm the gather the
// filter-gradient kernel assumes)
// ------------------------------------------------------------------------------------------
__global__ void selftest_tr16_kernel(short *out) {
    __shared__ __attribute__((aligned(16))) short lds[64 * 4];
    for (int i = threadIdx.x; i < 256; i += 64) lds[i] = (short)i;
    __syncthreads();
    s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(lds + threadIdx.x * 4));
    out[threadIdx.x * 4 + 0] = v[0];
    out[threadIdx.x * 4 + 1] = v[1];
    out[threadIdx.x * 4 + 2] = v[2];
    out[threadIdx.x * 4 + 3] = v[3];
}
extern "C" int yolo2_selftest_tr16(short *out, void *stream) {
    Y2_CHECK_ARG(out);
    selftest_tr16_kernel<<<1, 64, 0, (hipStream_t)stream>>>(out);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

// ---- test instrument: what an RCCL ring looks like to the dispatcher.  `workgroups` persistent 256-thread workgroups, each holding a
// whole CU (all 160 KiB of LDS), spin until *stop becomes non-zero or `max_us` microseconds have passed (bounded: a test can never hang
// the GPU on it).  *started counts the workgroups that are resident.  tests/test_streamk_occupied_gpu.py runs the stream-K convolutions
// beside it.
__global__ __launch_bounds__(256) void occupy_kernel(volatile int *stop, int *started, long max_ticks) {
    extern __shared__ unsigned char lds[];
    if (threadIdx.x == 0) {
        lds[0] = 1;
        __hip_atomic_fetch_add(started, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long t0 = wall_clock64();
        while (__hip_atomic_load(const_cast<int *>(stop), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0 && wall_clock64() - t0 < max_ticks) __builtin_amdgcn_s_sleep(32);
    }
    __syncthreads();
}
extern "C" int yolo2_debug_occupy(int workgroups, int *stop, int *started, int max_us, void *stream) {
    Y2_CHECK_ARG(workgroups > 0 && workgroups <= 256 && stop && started && max_us > 0 && max_us <= 2000000);
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(occupy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
            yolo2_set_error("yolo2_debug_occupy: cannot raise the dynamic LDS limit");
            return YOLO2_E_LAUNCH;
        }
        attr_set = true;
    }
    occupy_kernel<<<workgroups, 256, 160 * 1024, (hipStream_t)stream>>>(stop, started, (long)max_us * 100);      // wall_clock64 ticks at 100 MHz
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
