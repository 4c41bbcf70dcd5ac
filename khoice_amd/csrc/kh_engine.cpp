// khoice_amd — host side of libkhoice_hip.so: context, device memory pool, set handles,
// orchestration of the gfx950 kernels and the C ABI declared in include/khoice_hip.h.
// There is deliberately no CPU implementation of any operation in this library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <chrono>
#include <cmath>
#include <memory>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/khoice_hip.h"
#include "kh_engine.h"
#include "kh_launch.h"
#include "kh_skm_rec.h"

// ------------------------------------------------------------------------------ errors
static thread_local std::string g_last_error;

int kh_fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}
extern "C" const char* kh_last_error(void) { return g_last_error.c_str(); }

#define HIPCHK(expr)                                                                      \
    do {                                                                                  \
        hipError_t e__ = (expr);                                                          \
        if (e__ != hipSuccess)                                                            \
            return kh_fail(KH_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                           __FILE__, __LINE__);                                           \
    } while (0)
#define KHCHK(expr)                  \
    do {                             \
        int r__ = (expr);            \
        if (r__ != KH_OK) return r__; \
    } while (0)

// ------------------------------------------------------------------------------ pool
// Stream-ordered caching allocator: every user of a ctx runs on its single stream, so a
// block released by one operation can be handed to the next without synchronising.
void* Pool::alloc(size_t bytes, size_t* got) {
    if (bytes == 0) bytes = 256;
    size_t want = (bytes + 255) & ~(size_t)255;
    if (want > (1u << 20)) want = (want + (1u << 20) - 1) & ~(size_t)((1u << 20) - 1);
    auto it = free_.lower_bound(want);
    if (it != free_.end() && it->first <= want + want / 4 + (1u << 20)) {
        void* p = it->second;
        *got = it->first;
        cached_bytes -= it->first;
        free_.erase(it);
        return p;
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
        trim();
        e = hipMalloc(&p, want);
        if (e != hipSuccess) return nullptr;
    }
    total_bytes += want;
    *got = want;
    return p;
}
void Pool::release(void* p, size_t bytes) {
    free_.emplace(bytes, p);
    cached_bytes += bytes;
}
void Pool::trim() {
    for (auto& kv : free_) {
        (void)hipFree(kv.second);
        total_bytes -= kv.first;
    }
    free_.clear();
    cached_bytes = 0;
}

// KHOICE_DEBUG_POISON=<0..255> (tests): every block handed out, fresh or recycled, is filled with
// that byte first, so that no form can lean on what a block held before.  Read at every call, like
// the other knobs; unset, nothing is queued.  -1 = unset or not a byte.
static int debug_poison() {
    const char* e = getenv("KHOICE_DEBUG_POISON");
    if (!e || !*e) return -1;
    char* end = nullptr;
    const long v = strtol(e, &end, 0);
    return (*end || v < 0 || v > 255) ? -1 : (int)v;
}

DevBuf* kh_ctx::buf_alloc(size_t bytes) {
    size_t got = 0;
    void* p = pool.alloc(bytes, &got);
    if (!p) return nullptr;
    const int poison = debug_poison();
    if (poison >= 0) {
        // Every user of the block runs on `st`, which exists from kh_ctx_create on (no allocation
        // precedes it), so the fill is ordered before them and after the block's last user.
        if (hipMemsetAsync(p, poison, got, st) != hipSuccess) {
            pool.release(p, got);
            return nullptr;
        }
        stat.poisoned_bytes += got;
    }
    DevBuf* b = new DevBuf;
    b->p = p;
    b->bytes = got;
    b->refs = 1;
    b->ctx = this;
    live_bufs.fetch_add(1);
    return b;
}
void buf_ref(DevBuf* b) { if (b) b->refs.fetch_add(1); }
void buf_unref(DevBuf* b) {
    if (!b) return;
    if (b->refs.fetch_sub(1) == 1) {
        if (kh_ctx* c = b->ctx) {                           // borrowed buffers have no ctx
            if (!c->closed) {
                c->pool.release(b->p, b->bytes);
                c->live_bufs.fetch_sub(1);
            } else {                                        // set freed after kh_ctx_destroy
                (void)hipSetDevice(c->dev);
                (void)hipFree(b->p);
                if (c->live_bufs.fetch_sub(1) == 1) delete c;
            }
        }
        delete b;
    }
}
// scoped temporary
struct Tmp {
    DevBuf* b = nullptr;
    ~Tmp() { buf_unref(b); }
    void release() { buf_unref(b); b = nullptr; }   // ahead of the scope's end (stream-ordered, as every release)
    template <class T> T* as() const { return reinterpret_cast<T*>(b->p); }
};
#define TMP_ALLOC(tmp, ctx, bytes)                                                        \
    do {                                                                                  \
        (tmp).b = (ctx)->buf_alloc(bytes);                                                \
        if (!(tmp).b) return kh_fail(KH_E_NOMEM, "device allocation of %zu bytes failed", \
                                     (size_t)(bytes));                                    \
    } while (0)
// scoped pinned host staging (kh_ctx::pin_alloc / pin_release)
struct Pinned {
    kh_ctx* c;
    void* p = nullptr;
    size_t n = 0;
    ~Pinned() { if (p) c->pin_release(p, n); }
};
#define PIN_ALLOC(pin, bytes)                                                               \
    do {                                                                                    \
        (pin).p = (pin).c->pin_alloc(bytes, &(pin).n);                                      \
        if (!(pin).p) return kh_fail(KH_E_NOMEM, "pinned host allocation failed");         \
    } while (0)

void* kh_ctx::pin_alloc(size_t bytes, size_t* got) {
    bytes = (bytes + 4095) & ~(size_t)4095;
    auto it = pinned_free.lower_bound(bytes);
    void* p = nullptr;
    if (it != pinned_free.end() && it->first <= 4 * bytes) {
        p = it->second;
        *got = it->first;
        pinned_free.erase(it);
    } else {
        if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
        *got = bytes;
    }
    const int poison = debug_poison();   // a released staging block has no copy in flight: its user synchronised
    if (poison >= 0) {
        memset(p, poison, *got);
        stat.poisoned_bytes += *got;
    }
    return p;
}
void kh_ctx::pin_release(void* p, size_t bytes) {
    if (p) pinned_free.emplace(bytes, p);
}

// KHOICE_TRACE=1: host-side timeline of kh_exp1_run on stderr (diagnostics only)
#include <chrono>
static bool g_trace = getenv("KHOICE_TRACE") != nullptr;
static double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static double g_t_build_submitted = 0, g_t_build_synced = 0;

// ------------------------------------------------------------------------------ profiling
void kh_ctx::prof_begin(int cls) {
    if (!profile) return;
    ProfEvt ev;
    ev.cls = cls;
    auto take = [&](hipEvent_t* e) {   // events are recycled: creating one costs microseconds
        if (!free_events.empty()) { *e = free_events.back(); free_events.pop_back(); }
        else (void)hipEventCreate(e);
    };
    take(&ev.a);
    take(&ev.b);
    (void)hipEventRecord(ev.a, st);
    evts.push_back(ev);
}
void kh_ctx::prof_end() {
    if (!profile || evts.empty()) return;
    (void)hipEventRecord(evts.back().b, st);
}
void kh_ctx::prof_collect() {
    if (evts.empty()) return;
    (void)hipStreamSynchronize(st);
    for (auto& ev : evts) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) {
            cls_ms[ev.cls] += ms;
            cls_n[ev.cls] += 1;
        }
        free_events.push_back(ev.a);
        free_events.push_back(ev.b);
    }
    evts.clear();
}
static const char* kClsNames[KC_COUNT] = {"extract_hist", "bucket_plan", "extract_scatter",
                                          "bucket_sort_rle", "range_bounds", "setop", "histogram",
                                          "remix", "copy_in", "union_tagged", "skm_scatter",
                                          "skm_regroup", "skm_union", "skm_big", "skm_pack", "skm_phased", "bmp_build",
                                          "bmp_readout", "bmp_pivot", "bmp_cross", "bmp_count", "bmp_present", "bmp_member", "skm_cross",
                                          "read_masks", "read_fold", "bmp_group_masks", "read_lookup",
                                          "index_dir", "index_tag", "read_index", "index_member"};

// ------------------------------------------------------------------------------ ctx API
extern "C" int kh_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int kh_ctx_create(int device, kh_ctx** out) {
    if (!out) return kh_fail(KH_E_ARG, "kh_ctx_create: out is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return kh_fail(KH_E_HIP, "no HIP device available (%s); khoice_amd has no CPU fallback",
                       e == hipSuccess ? "0 devices" : hipGetErrorString(e));
    if (device < 0 || device >= n) return kh_fail(KH_E_ARG, "device %d out of range [0,%d)", device, n);
    HIPCHK(hipSetDevice(device));
    kh_ctx* c = new kh_ctx;
    c->dev = device;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    c->arch = prop.gcnArchName;
    c->cus = prop.multiProcessorCount;
    if (c->arch.find("gfx950") == std::string::npos && !getenv("KHOICE_ALLOW_ANY_ARCH")) {
        std::string a = c->arch;
        delete c;
        return kh_fail(KH_E_HIP, "device %d is %s; this library carries gfx950 code only", device,
                       a.c_str());
    }
    HIPCHK(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
    c->dynamic_order = getenv("KHOICE_TICKETS") != nullptr;   // see KhLookback::dynamic
    *out = c;
    return KH_OK;
}
extern "C" void kh_ctx_destroy(kh_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->dev);
    (void)hipStreamSynchronize(c->st);
    c->prof_collect();
    for (auto e : c->free_events) (void)hipEventDestroy(e);
    for (auto& kv : c->pinned_free) (void)hipHostFree(kv.second);
    c->pinned_free.clear();
    c->pool.trim();
    (void)hipStreamDestroy(c->st);
    c->st = nullptr;
    c->closed = true;
    if (c->live_bufs.load() == 0) delete c;
}
extern "C" int kh_sync(kh_ctx* c) {
    if (!c) return kh_fail(KH_E_ARG, "ctx is NULL");
    HIPCHK(hipStreamSynchronize(c->st));
    return KH_OK;
}
extern "C" int kh_trim(kh_ctx* c) {
    if (!c) return kh_fail(KH_E_ARG, "ctx is NULL");
    HIPCHK(hipStreamSynchronize(c->st));
    c->pool.trim();
    return KH_OK;
}
extern "C" int kh_profile_enable(kh_ctx* c, int on) {
    if (!c) return kh_fail(KH_E_ARG, "ctx is NULL");
    c->prof_collect();
    c->profile = on != 0;
    return KH_OK;
}
extern "C" int kh_stats_reset(kh_ctx* c) {
    if (!c) return kh_fail(KH_E_ARG, "ctx is NULL");
    c->prof_collect();
    for (int i = 0; i < KC_COUNT; ++i) { c->cls_ms[i] = 0; c->cls_n[i] = 0; }
    c->stat = Stats();
    return KH_OK;
}
extern "C" int kh_stats(kh_ctx* c, char* buf, size_t buflen) {
    if (!c || !buf) return kh_fail(KH_E_ARG, "kh_stats: NULL argument");
    c->prof_collect();
    std::string s = "{";
    char t[512];
    snprintf(t, sizeof t, "\"device\":%d,\"arch\":\"%s\",\"cus\":%d,", c->dev, c->arch.c_str(), c->cus);
    s += t;
    snprintf(t, sizeof t,
             "\"builds\":%llu,\"bases\":%llu,\"text_packed\":%llu,\"kmers\":%llu,\"distinct\":%llu,\"setops\":%llu,"
             "\"setop_in\":%llu,\"setop_out\":%llu,\"retries\":%llu,\"order_fallbacks\":%llu,\"skm_records\":%llu,\"big_slots\":%llu,\"cross_multi_slots\":%llu,\"poisoned_bytes\":%llu,\"pool_bytes\":%zu,",
             (unsigned long long)c->stat.builds, (unsigned long long)c->stat.bases,
             (unsigned long long)c->stat.text_packed,
             (unsigned long long)c->stat.kmers, (unsigned long long)c->stat.distinct,
             (unsigned long long)c->stat.setops, (unsigned long long)c->stat.setop_in,
             (unsigned long long)c->stat.setop_out, (unsigned long long)c->stat.retries,
             (unsigned long long)c->stat.order_fallbacks, (unsigned long long)c->stat.skm_records,
             (unsigned long long)c->stat.big_slots, (unsigned long long)c->stat.cross_multi_slots,
             (unsigned long long)c->stat.poisoned_bytes,
             c->pool.total_bytes);
    s += t;
    s += "\"kernels\":{";
    for (int i = 0; i < KC_COUNT; ++i) {
        snprintf(t, sizeof t, "%s\"%s\":{\"ms\":%.6f,\"launches\":%llu}", i ? "," : "", kClsNames[i],
                 c->cls_ms[i], (unsigned long long)c->cls_n[i]);
        s += t;
    }
    s += "}}";
    if (s.size() + 1 > buflen) return kh_fail(KH_E_ARG, "kh_stats: buffer too small (%zu needed)", s.size() + 1);
    memcpy(buf, s.c_str(), s.size() + 1);
    return KH_OK;
}

// ------------------------------------------------------------------------------ sets
extern "C" void kh_set_free(kh_set* s) {
    if (!s) return;
    buf_unref(s->kb);
    buf_unref(s->cb);
    delete s;
}
extern "C" int kh_set_info(const kh_set* s, uint64_t* n, int* k, int* w, int* has_counts,
                           uint32_t* uniform) {
    if (!s) return kh_fail(KH_E_ARG, "set is NULL");
    if (n) *n = s->n;
    if (k) *k = s->k;
    if (w) *w = s->W;
    if (has_counts) *has_counts = s->cb != nullptr;
    if (uniform) *uniform = s->uniform;
    return KH_OK;
}
static kh_set* make_set(int k, u64 n, DevBuf* kb, size_t koff, DevBuf* cb, size_t coff, u32 uniform,
                        u32 counter_max = KH_KMC_DEFAULT_CS) {
    kh_set* s = new kh_set;
    s->k = k;
    s->W = k <= 32 ? 1 : 2;
    s->n = n;
    s->kb = kb;
    s->koff = koff;
    s->cb = cb;
    s->coff = coff;
    s->uniform = uniform;
    s->counter_max = counter_max;
    return s;
}
static int check_k(int k) {
    if (k < 1 || k > 64) return kh_fail(KH_E_ARG, "k=%d outside the supported range 1..64", k);
    return KH_OK;
}

extern "C" int kh_set_counter_max(const kh_set* s, uint32_t* counter_max) {
    if (!s || !counter_max) return kh_fail(KH_E_ARG, "kh_set_counter_max: NULL argument");
    *counter_max = s->counter_max;
    return KH_OK;
}

extern "C" int kh_set_device_ptrs(const kh_set* s, const void** keys, const uint32_t** counts) {
    if (!s) return kh_fail(KH_E_ARG, "set is NULL");
    if (keys) *keys = s->n ? s->keys_ptr() : nullptr;
    if (counts) *counts = s->counts_ptr();
    return KH_OK;
}

extern "C" int kh_set_counts(kh_ctx* c, const kh_set* in, uint32_t value, kh_set** out) {
    if (!c || !in || !out) return kh_fail(KH_E_ARG, "kh_set_counts: NULL argument");
    if (value == 0) return kh_fail(KH_E_ARG, "set_counts 0 would empty the database");
    buf_ref(in->kb);
    *out = make_set(in->k, in->n, in->kb, in->koff, nullptr, 0, value, std::max<u32>(value, KH_KMC_DEFAULT_CS));
    return KH_OK;
}

#ifdef KH_STAMPS
void kh_debug_set_stamps(u64* p);
void kh_debug_set_stamps_skm(u64* p);
// diagnostic build: average shader-clock deltas between phase stamps over all workgroups
static void report_stamps(kh_ctx* c, const char* what, DevBuf* sb, u64 nparts) {
    std::vector<u64> h(nparts * 16);
    (void)hipMemcpyAsync(h.data(), sb->p, nparts * 128, hipMemcpyDeviceToHost, c->st);
    (void)hipStreamSynchronize(c->st);
    double sum[16] = {0};
    u64 cnt = 0, tmin = ~0ull, tmax = 0;
    for (u64 q = 0; q < nparts; ++q) {
        const u64* t = &h[q * 16];
        if (!t[0] || !t[8]) continue;
        ++cnt;
        for (int i = 1; i <= 8; ++i) if (t[i] && t[i - 1]) sum[i] += (double)(t[i] - t[i - 1]);
        tmin = std::min(tmin, t[0]);
        tmax = std::max(tmax, t[8]);
    }
    {   // optional finer stamps 9..11 inside the phase between stamps 4 and 5
        double s9 = 0, s10 = 0, s11 = 0; u64 c9 = 0;
        for (u64 q = 0; q < nparts; ++q) {
            const u64* t = &h[q * 16];
            if (!t[4] || !t[9] || !t[10] || !t[11] || !t[5]) continue;
            ++c9; s9 += (double)(t[9] - t[4]); s10 += (double)(t[10] - t[9]); s11 += (double)(t[11] - t[10]);
        }
        if (c9) fprintf(stderr, "[stamps] %s inside 4-5: first-probe %.0f rounds %.0f stores %.0f (then barrier)\n", what, s9 / c9, s10 / c9, s11 / c9);
    }
    fprintf(stderr, "[stamps] %s parts=%llu span=%.0f cyc | load %.0f count %.0f scan %.0f scatter %.0f insert %.0f walk1 %.0f lookback %.0f walk2 %.0f\n",
            what, (unsigned long long)cnt, (double)(tmax - tmin), sum[1] / cnt, sum[2] / cnt, sum[3] / cnt, sum[4] / cnt,
            sum[5] / cnt, sum[6] / cnt, sum[7] / cnt, sum[8] / cnt);
    {   // every stamp as an offset from stamp 0 (order-free: stamps 9..15 may sit anywhere)
        std::string line;
        for (int i = 1; i < 16; ++i) {
            double s2 = 0; u64 c2 = 0;
            for (u64 q = 0; q < nparts; ++q) {
                const u64* t = &h[q * 16];
                if (!t[0] || !t[i]) continue;
                ++c2; s2 += (double)((long long)(t[i] - t[0]));
            }
            if (c2) { char b[64]; snprintf(b, sizeof b, " t%d=%.0f(n=%llu)", i, s2 / c2, (unsigned long long)c2); line += b; }
        }
        fprintf(stderr, "[stamps] %s offsets from t0:%s\n", what, line.c_str());
    }
    // $KHOICE_STAMP_DUMP: every part's sixteen words, one line per part, appended (tools/union_stamps.py reads the
    // union's: words 12 and 13 are the workgroup + 1 and the slot's place in its walk)
    if (const char* path = getenv("KHOICE_STAMP_DUMP")) {
        if (FILE* f = fopen(path, "a")) {
            fprintf(f, "# %s\n", what);
            for (u64 q = 0; q < nparts; ++q) {
                fprintf(f, "%llu", (unsigned long long)q);
                for (int i = 0; i < 16; ++i) fprintf(f, " %llu", (unsigned long long)h[q * 16 + i]);
                fprintf(f, "\n");
            }
            fclose(f);
        }
    }
}
#ifdef KH_STAMPS_WG
void kh_debug_set_stamps_skm2(u64* p);
// -DKH_STAMPS_WG: when every workgroup of the persistent union began and ended its walk, one line per workgroup
// appended to $KHOICE_WG_DUMP (tools/wg_ends.py reads it): call, workgroup, hardware id, XCC, shader clock at the
// beginning and the end, constant-rate clock at the beginning and the end
// ($KHOICE_WG_DUMP_SCATTER: the same for the workgroups of k_skm_scatter, a tile each)
static void dump_wg_ends(kh_ctx* c, DevBuf* sb, u32 grid, bool scatter = false) {
    const char* path = getenv(scatter ? "KHOICE_WG_DUMP_SCATTER" : "KHOICE_WG_DUMP");
    if (!path) return;
    static int calls[2] = {0, 0};
    int& call = calls[scatter];
    std::vector<u64> h((size_t)grid * 16);
    (void)hipMemcpyAsync(h.data(), sb->p, (size_t)grid * 128, hipMemcpyDeviceToHost, c->st);
    (void)hipStreamSynchronize(c->st);
    FILE* f = fopen(path, "a");
    if (!f) return;
    for (u32 b = 0; b < grid; ++b) {
        const u64* t = &h[(size_t)b * 16];
        fprintf(f, "%d %u %llu %llu %llu %llu %llu %llu\n", call, b, (unsigned long long)t[1], (unsigned long long)t[2],
                (unsigned long long)t[0], (unsigned long long)t[8], (unsigned long long)t[3], (unsigned long long)t[11]);
    }
    fclose(f);
    ++call;
}
#endif
#endif

// The texts of a run on the device (build_once, skm_prepare, BmpRun): a text that is resident and 16-byte aligned is
// read in place, every other one is packed into d_seq at a multiple of 16 bytes, with 256 bytes behind the last (16-byte
// loads may run past the last base).
struct TextStage {
    Tmp d_seq;                      // the packed copy (256 bytes when every text is read in place)
    std::vector<const u8*> dev;     // text i on the device
    // text i is seqs[perm ? perm[i] : i].  The copies are queued on the context's stream (inside the caller's KC_COPY_IN)
    // and counted in text_packed.
    int copy_in(kh_ctx* c, int n, const uint8_t* const* seqs, const uint64_t* lens, int on_device, const int* perm = nullptr) {
        auto in_place = [&](const uint8_t* p) { return on_device && (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
        std::vector<u64> pack_off(n);
        u64 seq_bytes = 0;
        bool need_pack = false;
        for (int i = 0; i < n; ++i) {
            const int t = perm ? perm[i] : i;
            pack_off[i] = seq_bytes;
            seq_bytes += (lens[t] + 15) & ~15ull;
            if (!in_place(seqs[t])) need_pack = true;
        }
        TMP_ALLOC(d_seq, c, need_pack ? seq_bytes + 256 : 256);
        dev.resize(n);
        for (int i = 0; i < n; ++i) {
            const int t = perm ? perm[i] : i;
            if (in_place(seqs[t])) { dev[i] = seqs[t]; continue; }
            dev[i] = d_seq.as<u8>() + pack_off[i];
            if (!lens[t]) continue;
            HIPCHK(hipMemcpyAsync(d_seq.as<u8>() + pack_off[i], seqs[t], lens[t],
                                  on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->st));
            c->stat.text_packed += lens[t];
        }
        return KH_OK;
    }
};

// ------------------------------------------------------------------------------ K1 build
// What a grid-mode build (KhGrid, kh_launch.h) leaves behind: nothing has been synchronised when
// build_once returns, the caller queues the tagged union behind it and waits once.
struct GridBuild {
    kh_ctx* c = nullptr;
    u32 fan = 1;            // in: largest group (sets the slot fill of the tagged union)
    u32 cap = 0;            // in: slot capacity of the tagged union
    double s_scale = 1.0;       // in: more sub-ranges per bucket than the estimate (retry after a slot overflow)
    u32 wave = 0, nwaves = 1;   // in: key-range wave (KhSeg::nb_virtual / b_first): this build keeps slice `wave` of `nwaves`
    u32 nb = 0, S = 0, nb_total = 0;
    u64 total_pos = 0, bases = 0, key_cap = 0;   // key_cap: records the key arrays of this build can hold
    DevBuf *okeys = nullptr, *bstart = nullptr, *off = nullptr, *distinct = nullptr, *lb = nullptr;
    void* pin = nullptr;    // plan staging: must outlive the asynchronous upload
    size_t pin_bytes = 0;
    ~GridBuild() {
        buf_unref(okeys); buf_unref(bstart); buf_unref(off); buf_unref(distinct); buf_unref(lb);
        if (pin && c) c->pin_release(pin, pin_bytes);
    }
};

static int build_once(kh_ctx* c, int nseq, const uint8_t* const* seqs, const uint64_t* lens,
                      int on_device, int k, u32 ci, u32 cx, u32 cs, int with_counts, u32 mean,
                      kh_set** out_sets, bool* capacity_hit, bool* order_retry, GridBuild* grid = nullptr) {
    const int W = k <= 32 ? 1 : 2;
    const size_t kb = 8 * (size_t)W;
    hipStream_t st = c->st;
    *capacity_hit = false;
    *order_retry = false;

    // ---- segment layout
    std::vector<KhSeg> segs(nseq);
    std::vector<KhTile> tiles;
    u64 total_pos = 0, thist_n = 0, bases = 0;
    u32 nb_total = 0, max_nb = 1;
    // Positions per extraction workgroup (tile): 65536 amortises the cursor rows best, but a small
    // batch (the per-call path: one 5 Mbp genome is 77 such tiles on 256 CUs) is cut finer so that
    // passes A and B fill the chip — down to one staging round of pass B.
    u32 tile_pos = KH_TILE;
    {
        u64 all_pos = 0;
        for (int i = 0; i < nseq; ++i) all_pos += lens[i] >= (u64)k ? lens[i] - k + 1 : 0;
        const u64 want_tiles = 4ull * (u64)std::max(1, c->cus);
        while (tile_pos > 2 * KH_SUBTILE && (all_pos + tile_pos - 1) / tile_pos < want_tiles) tile_pos >>= 1;
        if (const char* ev = getenv("KHOICE_TILE_POS")) tile_pos = std::max<u32>(2 * KH_SUBTILE, (u32)strtoul(ev, nullptr, 10) / (2 * KH_SUBTILE) * (2 * KH_SUBTILE));
    }
    u64 grid_nb = 1;   // grid mode: one bucket grid for every sequence, sized by the longest
    const u32 nwaves = grid ? std::max<u32>(1, grid->nwaves) : 1u;
    if (grid) {
        const u64 per = (u64)mean * nwaves;   // a wave keeps 1/nwaves of every genome's keys
        for (int i = 0; i < nseq; ++i)
            if (lens[i] >= (u64)k) grid_nb = std::max<u64>(grid_nb, (lens[i] - k + 1 + per - 1) / per);
    }
    for (int i = 0; i < nseq; ++i) {
        KhSeg& s = segs[i];
        s.seq = nullptr;
        s.len = lens[i];
        s.npos = lens[i] >= (u64)k ? lens[i] - k + 1 : 0;
        const u64 want_b = grid ? grid_nb : std::max<u64>(1, (s.npos + mean - 1) / mean);
        if (want_b > KH_MAX_BUCKETS_PER_SEG)
            return kh_fail(KH_E_ARG,
                           "sequence %d has %llu k-mer positions; at most %llu per sequence are "
                           "supported by this build",
                           i, (unsigned long long)s.npos,
                           (unsigned long long)KH_MAX_BUCKETS_PER_SEG * mean);
        s.nbuckets = (u32)want_b;
        s.nb_virtual = (u32)want_b * nwaves;
        s.b_first = grid ? grid->wave * (u32)want_b : 0u;
        s.bucket_base = nb_total;
        s.ntiles = (u32)((s.npos + tile_pos - 1) / tile_pos);
        s.tile_base = (u32)tiles.size();
        s.thist_base = thist_n;
        for (u32 t = 0; t < s.ntiles; ++t) tiles.push_back(KhTile{(u32)i, t});
        thist_n += (u64)s.ntiles * s.nbuckets;
        nb_total += s.nbuckets;
        max_nb = std::max(max_nb, s.nbuckets);
        total_pos += s.npos;
        bases += lens[i];
    }
    const u32 ntiles = (u32)tiles.size();
    const u32 nb_alloc = (max_nb + 3) & ~3u;

    // ---- device buffers
    Tmp d_thist, d_tot, d_bstart, d_part, d_lb;
    TMP_ALLOC(d_thist, c, 4 * std::max<u64>(1, thist_n));
    TMP_ALLOC(d_tot, c, 8 * (u64)nb_total);
    TMP_ALLOC(d_bstart, c, 8 * ((u64)nb_total + 1));
    Tmp d_scan;
    TMP_ALLOC(d_scan, c, 8 * kh_exscan_tmp_words(nb_total));
    // a key-range wave keeps about total_pos / nwaves keys — how many exactly is known after the
    // bucket plan, so its partition and output arrays are allocated there (one extra wait per wave)
    const bool late_alloc = nwaves > 1;
    u64 key_cap = std::max<u64>(1, total_pos);
    if (!late_alloc) TMP_ALLOC(d_part, c, kb * key_cap);
    TMP_ALLOC(d_lb, c, 8 * (u64)nb_total + 64);
    KhGrid kgrid{nullptr, nullptr, 0, 0};
    if (grid) {
        // sub-ranges per bucket: the tagged union's slot = one sub-range of one bucket in every
        // genome; fill T with T + 5 sigma <= capacity, sigma <= sqrt(T * fan) (copies of one key
        // inside a group arrive together; setop_prepare has the same rule)
        const double zg = 5.0 * std::sqrt((double)std::max<u32>(1, grid->fan));
        const double x = 0.5 * (-zg + std::sqrt(zg * zg + 4.0 * (double)grid->cap));
        const u64 target = std::max<u64>(16, std::min<u64>((u64)grid->cap * 92 / 100, (u64)(x * x)));
        const u64 per_bucket = (total_pos + grid_nb * nwaves - 1) / (grid_nb * nwaves);   // keys of one bucket over all genomes
        grid->S = (u32)std::max<u64>(1, (u64)std::ceil((double)((per_bucket + target - 1) / target) * grid->s_scale));
        if (grid->S > (u32)KH_FINE_BINS / 2 || grid_nb * grid->S > 0x7fffffffull)
            return kh_fail(KH_E_ARG, "grid build: %llu sub-ranges per bucket", (unsigned long long)grid->S);
        grid->c = c;
        grid->nb = (u32)grid_nb;
        grid->nb_total = nb_total;
        grid->total_pos = total_pos;
        grid->bases = bases;
        grid->off = c->buf_alloc(2 * (size_t)nb_total * (grid->S + 1));
        grid->distinct = c->buf_alloc(8 * (size_t)nseq);
        if (!grid->off || !grid->distinct) return kh_fail(KH_E_NOMEM, "device allocation failed (bucket index)");
        HIPCHK(hipMemsetAsync(grid->distinct->p, 0, 8 * (size_t)nseq, st));
        kgrid = KhGrid{reinterpret_cast<u16*>(grid->off->p), reinterpret_cast<unsigned long long*>(grid->distinct->p),
                       grid->S, grid->nb};
    }
    DevBuf* okeys = late_alloc ? nullptr : c->buf_alloc(kb * key_cap);
    if (!late_alloc && !okeys) return kh_fail(KH_E_NOMEM, "device allocation failed (output keys)");
    DevBuf* ocnt = nullptr;
    if (with_counts) {
        ocnt = c->buf_alloc(4 * std::max<u64>(1, total_pos));
        if (!ocnt) { buf_unref(okeys); return kh_fail(KH_E_NOMEM, "device allocation failed (counts)"); }
    }
    struct Guard { DevBuf *&a, *&b; ~Guard() { buf_unref(a); buf_unref(b); } } guard{okeys, ocnt};

    TextStage texts;
    c->prof_begin(KC_COPY_IN);
    KHCHK(texts.copy_in(c, nseq, seqs, lens, on_device));
    for (int i = 0; i < nseq; ++i) segs[i].seq = texts.dev[i];
    // Start order of pass C (KhBucketWork): buckets of up to 64 consecutive segments are
    // interleaved (bucket 0 of each, bucket 1 of each, ...), every segment writes into its own
    // output region [out_base, out_base + npos) and runs its own look-back chain.
    Pinned plan_pin{c};
    // the launch sequence's small tables — output bases, start ranks, segments, tiles — travel in ONE upload
    // (three separate copies, two of them from pageable vectors, were a sixth of a single-genome build)
    const size_t up_rank = 8 * (size_t)nseq, up_segs = (up_rank + 4 * (size_t)nb_total + 7) & ~(size_t)7,
                 up_tiles = up_segs + sizeof(KhSeg) * (size_t)nseq,
                 up_bytes = up_tiles + sizeof(KhTile) * (size_t)std::max<u32>(1, ntiles);
    PIN_ALLOC(plan_pin, up_bytes);
    u64* h_out_base = static_cast<u64*>(plan_pin.p);
    u32* h_rank = reinterpret_cast<u32*>(h_out_base + nseq);
    memcpy(static_cast<u8*>(plan_pin.p) + up_segs, segs.data(), sizeof(KhSeg) * (size_t)nseq);
    if (ntiles) memcpy(static_cast<u8*>(plan_pin.p) + up_tiles, tiles.data(), sizeof(KhTile) * (size_t)ntiles);
    {
        u64 ob = 0;
        u32 next = 0;
        for (int i = 0; i < nseq; ++i) { h_out_base[i] = ob; ob += segs[i].npos; }
        for (int s0 = 0; s0 < nseq; s0 += 64) {
            const int s1 = std::min(nseq, s0 + 64);
            u32 deepest = 0;
            for (int i = s0; i < s1; ++i) deepest = std::max(deepest, segs[i].nbuckets);
            for (u32 b = 0; b < deepest; ++b)
                for (int i = s0; i < s1; ++i)
                    if (b < segs[i].nbuckets) h_rank[segs[i].bucket_base + b] = next++;
        }
    }
    Tmp d_plan, d_work;
    TMP_ALLOC(d_plan, c, up_bytes);
    TMP_ALLOC(d_work, c, sizeof(KhBucketWork) * (size_t)nb_total);
    HIPCHK(hipMemcpyAsync(d_plan.b->p, plan_pin.p, up_bytes, hipMemcpyHostToDevice, st));
    const u64* d_out_base = d_plan.as<u64>();
    const u32* d_rank = reinterpret_cast<const u32*>(d_out_base + nseq);
    const KhSeg* d_segs_p = reinterpret_cast<const KhSeg*>(d_plan.as<u8>() + up_segs);
    const KhTile* d_tiles_p = reinterpret_cast<const KhTile*>(d_plan.as<u8>() + up_tiles);
    c->prof_end();

    // ---- pass A, bucket plan, pass B
    c->prof_begin(KC_EXTRACT_HIST);
    kh_launch_extract(W, false, texts.d_seq.as<u8>(), d_segs_p, d_tiles_p, ntiles,
                      nb_alloc, k, d_thist.as<u32>(), nullptr, nullptr, tile_pos, st);
    c->prof_end();
    c->prof_begin(KC_BUCKET_PLAN);
    kh_launch_col_totals(d_segs_p, nseq, max_nb, d_thist.as<u32>(), d_tot.as<u64>(), st);
    kh_launch_exscan(d_tot.as<u64>(), d_bstart.as<u64>(), nb_total, d_scan.as<u64>(), st);
    Tmp d_over;   // grid mode: list of the buckets above the LDS capacity
    if (grid) {
        TMP_ALLOC(d_over, c, 4 * ((size_t)nb_total + 1));
        HIPCHK(hipMemsetAsync(d_over.b->p, 0, 4, st));
    }
    kh_launch_col_offsets(d_segs_p, nseq, max_nb, d_thist.as<u32>(), d_bstart.as<u64>(), d_rank,
                          d_out_base, d_work.as<KhBucketWork>(), grid ? d_over.as<u32>() : nullptr,
                          grid ? kh_grid_bucket_capacity(W) : 0u, st);
    c->prof_end();
    if (late_alloc) {
        u64 nkeys = 0;
        HIPCHK(hipMemcpyAsync(&nkeys, d_bstart.as<u64>() + nb_total, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        key_cap = std::max<u64>(1, nkeys);
        TMP_ALLOC(d_part, c, kb * key_cap);
        okeys = c->buf_alloc(kb * key_cap);
        if (!okeys) return kh_fail(KH_E_NOMEM, "device allocation failed (output keys)");
    }
#ifdef KH_STAMPS
    Tmp d_stamps_b;
    TMP_ALLOC(d_stamps_b, c, 128 * (u64)std::max<u32>(1, ntiles));
    HIPCHK(hipMemsetAsync(d_stamps_b.b->p, 0, 128 * (u64)std::max<u32>(1, ntiles), st));
    kh_debug_set_stamps(d_stamps_b.as<u64>());
#endif
    c->prof_begin(KC_EXTRACT_SCATTER);
    kh_launch_extract(W, true, texts.d_seq.as<u8>(), d_segs_p, d_tiles_p, ntiles,
                      nb_alloc, k, d_thist.as<u32>(), d_bstart.as<u64>(), d_part.b->p, tile_pos, st);
    c->prof_end();
#ifdef KH_STAMPS
    report_stamps(c, "extract_scatter (last round of a tile: decode / extract / scan / place / flush / - / - / cursors)", d_stamps_b.b, ntiles);
    kh_debug_set_stamps(nullptr);
#endif

    // ---- pass C
    KhLookback lb;
    lb.desc = d_lb.as<u64>();
    lb.ticket = reinterpret_cast<u32*>(d_lb.as<u64>() + nb_total);
    lb.err = lb.ticket + 1;
    lb.dynamic = c->dynamic_order ? 1u : 0u;
    HIPCHK(hipMemsetAsync(d_lb.b->p, 0, 8 * (u64)nb_total + 64, st));
#ifdef KH_STAMPS
    Tmp d_stamps;
    TMP_ALLOC(d_stamps, c, 128 * (u64)nb_total);
    HIPCHK(hipMemsetAsync(d_stamps.b->p, 0, 128 * (u64)nb_total, st));
    kh_debug_set_stamps(d_stamps.as<u64>());
#endif
    c->prof_begin(KC_BUCKET_SORT);
    if (grid)
        kh_launch_grid_bucket(W, d_part.b->p, d_work.as<KhBucketWork>(), nb_total, k, okeys->p, d_over.as<u32>(), lb.err,
                              kgrid, st);
    else
        kh_launch_bucket_sort(W, d_part.b->p, d_work.as<KhBucketWork>(), nb_total, k, okeys->p,
                              ocnt ? reinterpret_cast<u32*>(ocnt->p) : nullptr, lb, ci, cx, cs, st);
    c->prof_end();
    HIPCHK(hipGetLastError());
#ifdef KH_STAMPS
    report_stamps(c, "bucket_sort", d_stamps.b, nb_total);
    kh_debug_set_stamps(nullptr);
#endif
    if (grid) {   // hand the device state over; the caller synchronises
        grid->key_cap = key_cap;
        buf_ref(okeys); grid->okeys = okeys;
        buf_ref(d_bstart.b); grid->bstart = d_bstart.b;
        buf_ref(d_lb.b); grid->lb = d_lb.b;
        grid->pin = plan_pin.p; grid->pin_bytes = plan_pin.n;
        plan_pin.p = nullptr;
        return KH_OK;
    }

    // ---- read back set boundaries
    if (g_trace) g_t_build_submitted = now_ms();
    Pinned pin{c};
    PIN_ALLOC(pin, 8 * (size_t)nb_total + 64 + 8);
    u64* desc = static_cast<u64*>(pin.p);
    u64& nvalid = desc[(size_t)nb_total + 8];
    HIPCHK(hipMemcpyAsync(desc, d_lb.b->p, 8 * (u64)nb_total + 64, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&nvalid, d_bstart.as<u64>() + nb_total, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (g_trace) g_t_build_synced = now_ms();
    const u32 err = reinterpret_cast<const u32*>(&desc[nb_total])[1];
    if (err & KH_ERR_SPIN_TIMEOUT) {
        if (c->dynamic_order) return kh_fail(KH_E_INTERNAL, "look-back spin timed out in bucket sort");
        c->dynamic_order = true;          // index order did not hold: tickets from now on
        c->stat.order_fallbacks++;
        *order_retry = true;              // same batch again with the same plan
        return KH_OK;
    }
    if (err & KH_ERR_CAPACITY) { *capacity_hit = true; return KH_OK; }
    c->stat.kmers += nvalid;
    c->stat.bases += bases;      // counted once per successful build, not per attempt

    for (int i = 0; i < nseq; ++i) {   // a segment's chain ends with its inclusive total
        const u64 n = desc[segs[i].bucket_base + segs[i].nbuckets - 1] & ((1ull << 62) - 1);
        buf_ref(okeys);
        if (ocnt) buf_ref(ocnt);
        out_sets[i] = make_set(k, n, okeys, h_out_base[i] * kb, ocnt, h_out_base[i] * 4, 1, cs);
        c->stat.distinct += n;
    }
    c->stat.builds += nseq;
    return KH_OK;
}

static int build_batch_plain(kh_ctx* c, int nseq, const uint8_t* const* seqs, const uint64_t* lens,
                             int on_device, int k, u32 ci, u32 cx, u32 cs, int with_counts,
                             kh_set** out_sets) {
    u32 mean = k <= 32 ? KH_BUCKET_MEAN_W1 : KH_BUCKET_MEAN_W2;
    u64 max_pos = 0;
    for (int i = 0; i < nseq; ++i)
        if (lens[i] >= (u64)k) max_pos = std::max<u64>(max_pos, lens[i] - k + 1);
    for (int attempt = 0; attempt < 6; ++attempt) {
        bool cap = false, again = false;
        for (int i = 0; i < nseq; ++i) out_sets[i] = nullptr;
        int r = build_once(c, nseq, seqs, lens, on_device, k, ci, cx, cs, with_counts, mean, out_sets, &cap, &again);
        if (r != KH_OK) return r;
        if (again) continue;              // look-back order fallback: nothing overflowed, same plan
        if (!cap) return KH_OK;
        c->stat.retries++;
        // more buckets, but never more than one segment's cursor table holds
        const u32 floor_mean = (u32)std::max<u64>(64, (max_pos + KH_MAX_BUCKETS_PER_SEG - 1) / KH_MAX_BUCKETS_PER_SEG);
        const u32 next = std::max<u32>(floor_mean, mean / 4);
        if (next >= mean) break;
        mean = next;
    }
    return kh_fail(KH_E_CAPACITY, "a bucket still holds more distinct k-mers than fit in LDS after re-planning");
}

extern "C" int kh_build_batch(kh_ctx* c, int nseq, const uint8_t* const* seqs, const uint64_t* lens,
                              int on_device, int k, uint32_t ci, uint32_t cx, uint32_t cs,
                              int with_counts, kh_set** out_sets) {
    if (!c || !seqs || !lens || !out_sets || nseq <= 0) return kh_fail(KH_E_ARG, "kh_build_batch: bad argument");
    KHCHK(check_k(k));
    if (ci < 1) ci = 1;
    if (cs < 1) return kh_fail(KH_E_ARG, "cs must be >= 1");
    HIPCHK(hipSetDevice(c->dev));
    // A sequence whose k-mer positions exceed what one segment's bucket table covers (the cursor
    // table of pass A/B lives in LDS) is cut into chunks that overlap by k-1 bases: every k-mer
    // start position belongs to exactly one chunk, so the chunk databases add up exactly.
    const u32 mean = k <= 32 ? KH_BUCKET_MEAN_W1 : KH_BUCKET_MEAN_W2;
    u64 chunk_pos = (u64)(KH_MAX_BUCKETS_PER_SEG / 4) * mean;
    if (const char* e = getenv("KHOICE_MAX_SEG_POS")) chunk_pos = std::max<u64>(64, strtoull(e, nullptr, 10));
    bool any_long = false;
    for (int i = 0; i < nseq; ++i)
        if (lens[i] >= (u64)k && lens[i] - k + 1 > chunk_pos) any_long = true;
    if (!any_long) return build_batch_plain(c, nseq, seqs, lens, on_device, k, ci, cx, cs, with_counts, out_sets);
    if (ci > 1 || cx != KH_NO_MAX)
        return kh_fail(KH_E_ARG, "-ci/-cx cut-offs are not supported for sequences of more than %llu k-mer positions",
                       (unsigned long long)chunk_pos);
    std::vector<const uint8_t*> cseq;
    std::vector<uint64_t> clen;
    std::vector<int> first(nseq + 1, 0);
    for (int i = 0; i < nseq; ++i) {
        first[i] = (int)cseq.size();
        const u64 npos = lens[i] >= (u64)k ? lens[i] - k + 1 : 0;
        if (npos <= chunk_pos) { cseq.push_back(seqs[i]); clen.push_back(lens[i]); continue; }
        for (u64 p = 0; p < npos; p += chunk_pos) {
            const u64 np = std::min(chunk_pos, npos - p);
            cseq.push_back(seqs[i] + p);
            clen.push_back(np + k - 1);
        }
    }
    first[nseq] = (int)cseq.size();
    std::vector<kh_set*> csets(cseq.size(), nullptr);
    auto cleanup = [&]() { for (auto* s : csets) kh_set_free(s); };
    // chunk databases keep exact counters (no saturation) until they are added up
    int r = build_batch_plain(c, (int)cseq.size(), cseq.data(), clen.data(), on_device, k, 1, KH_NO_MAX,
                              with_counts ? 0x7fffffffu : cs, with_counts, csets.data());
    if (r != KH_OK) { cleanup(); return r; }
    for (int i = 0; i < nseq; ++i) out_sets[i] = nullptr;
    for (int i = 0; i < nseq && r == KH_OK; ++i) {
        const int m = first[i + 1] - first[i];
        if (m == 1) { out_sets[i] = csets[first[i]]; csets[first[i]] = nullptr; continue; }
        kh_set* u = nullptr;
        r = kh_union_sum(c, csets.data() + first[i], m, with_counts ? cs : 0x7fffffffu, &u, nullptr, 0);
        if (r != KH_OK) break;
        if (with_counts) { out_sets[i] = u; continue; }
        r = kh_set_counts(c, u, 1, &out_sets[i]);     // plain set: every counter 1
        kh_set_free(u);
    }
    if (r != KH_OK) for (int i = 0; i < nseq; ++i) { kh_set_free(out_sets[i]); out_sets[i] = nullptr; }
    cleanup();
    return r;
}

// ------------------------------------------------------------------------------ set ops
// One set operation as an asynchronous job: setop_launch() only enqueues work on the ctx stream
// (kernels + the small device-to-host copies of the result size / histogram); setop_finish()
// is called after a stream synchronisation, turns the result into a handle and re-plans with
// smaller slots in the (rare) case a slot overflowed LDS.  Independent operations can thus be
// enqueued back to back and share one synchronisation (kh_exp1_run does that for the groups).
struct SetopJob {
    kh_ctx* c = nullptr;
    std::vector<const kh_set*> in;
    int op = 0, mode = 0, k = 0, W = 1;
    u32 cs = 0, hist_len = 0, cap = 0, nranges = 0;
    uint64_t* hist = nullptr;
    bool pay = false, empty = false;
    bool hist_only = false;   // nobody reads the output as one array: may run as several chains
    u64 total = 0, target = 0;
    DevBuf *okeys = nullptr, *ocnt = nullptr, *d_views = nullptr, *d_bounds = nullptr, *d_lb = nullptr;
    // pinned staging, mirroring the device workspace from its last descriptor on:
    // [last descriptor: 1 x u64][control: 8 x u64 = ticket, err | fullest slot | ...][hist][views]
    void* pin = nullptr;
    size_t pin_bytes = 0;
    u64* tail = nullptr;
    u64* pin_hist = nullptr;
    KhSetView* views = nullptr;
    u64 lb_words() const { return (u64)nranges + 8 + (hist ? hist_len : 0); }
    ~SetopJob() {
        buf_unref(okeys); buf_unref(ocnt); buf_unref(d_views); buf_unref(d_bounds); buf_unref(d_lb);
        if (pin && c) c->pin_release(pin, pin_bytes);
    }
};
#define JOB_ALLOC(field, bytes)                                                              \
    do {                                                                                     \
        buf_unref(j.field);                                                                  \
        j.field = c->buf_alloc(bytes);                                                       \
        if (!j.field) return kh_fail(KH_E_NOMEM, "device allocation of %zu bytes failed", (size_t)(bytes)); \
    } while (0)

static int setop_prepare(SetopJob& j) {
    kh_ctx* c = j.c;
    const int nsets = (int)j.in.size();
    j.k = j.in[0]->k;
    j.W = j.in[0]->W;
    for (auto* s : j.in)
        if (s->k != j.k) return kh_fail(KH_E_KMISMATCH, "operands built with different k (%d vs %d)", j.k, s->k);
    j.pay = !(j.op == KH_OP_UNION && j.mode == KH_OC_SUM);
    j.total = 0;
    if (!j.pin) {
        j.pin = c->pin_alloc(72 + 8 * (size_t)j.hist_len + sizeof(KhSetView) * nsets, &j.pin_bytes);
        if (!j.pin) return kh_fail(KH_E_NOMEM, "pinned host allocation failed");
        j.tail = static_cast<u64*>(j.pin);
        j.pin_hist = j.tail + 9;
        j.views = reinterpret_cast<KhSetView*>(j.pin_hist + j.hist_len);
    }
    j.tail[0] = j.tail[1] = j.tail[2] = j.tail[3] = 0;
    KhSetView* views = j.views;
    for (int g = 0; g < nsets; ++g) {
        views[g].keys = j.in[g]->n ? j.in[g]->keys_ptr() : nullptr;
        views[g].counts = j.in[g]->counts_ptr();
        views[g].n = j.in[g]->n;
        views[g].uniform = j.in[g]->uniform;
        views[g].pad = 0;
        if (j.in[g]->cb || j.in[g]->uniform != 1) j.pay = true;
        j.total += j.in[g]->n;
    }
    c->stat.setops++;
    c->stat.setop_in += j.total;
    j.empty = j.total == 0;
    if (j.empty) return KH_OK;
    j.cap = j.W == 1 ? (j.pay ? KH_SORT_CAP_PAY_W1 : KH_SORT_CAP_W1) : (j.pay ? KH_SORT_CAP_PAY_W2 : KH_SORT_CAP_W2);
    // Mean slot fill T: a slot holds a Poisson number of distinct keys, each up to G = nsets
    // times, so its size has sigma <= sqrt(T * G); T is the largest fill with T + 5 sigma <= cap
    // (G = 5: 84 % of cap, G = 10: 78 %, G = 128: 42 %; 90 % at G = 5 was measured to re-plan).
    {
        const double zg = 5.0 * std::sqrt((double)std::max(1, nsets));
        const double x = 0.5 * (-zg + std::sqrt(zg * zg + 4.0 * (double)j.cap));
        j.target = std::max<u64>(16, std::min<u64>((u64)j.cap * 92 / 100, (u64)(x * x)));
    }
    JOB_ALLOC(okeys, 8 * (size_t)j.W * j.total);
    JOB_ALLOC(ocnt, 4 * j.total);
    JOB_ALLOC(d_views, sizeof(KhSetView) * nsets);
    HIPCHK(hipMemcpyAsync(j.d_views->p, views, sizeof(KhSetView) * nsets, hipMemcpyHostToDevice, c->st));
    return KH_OK;
}

// plan: number of slots and the per-launch workspaces
static int setop_plan(SetopJob& j) {
    kh_ctx* c = j.c;
    if (j.empty) return KH_OK;
    const int nsets = (int)j.in.size();
    const u64 nr64 = std::max<u64>(1, (j.total + j.target - 1) / j.target);
    if (nr64 > 0x7fffffffull) return kh_fail(KH_E_ARG, "set operation too large for one launch");
    j.nranges = (u32)nr64;
    JOB_ALLOC(d_bounds, 8 * ((u64)j.nranges + 1) * nsets);
    // one workspace: [descriptors: nranges][control: 64 B][histogram: hist_len], zeroed by the
    // range-bounds kernel and read back (from the last descriptor on) with one copy
    JOB_ALLOC(d_lb, 8 * j.lb_words());
    return KH_OK;
}

static KhBoundsJob setop_bounds_job(const SetopJob& j) {
    return KhBoundsJob{reinterpret_cast<const KhSetView*>(j.d_views->p), reinterpret_cast<u64*>(j.d_bounds->p),
                       reinterpret_cast<u64*>(j.d_lb->p), j.lb_words(), (u32)j.in.size(), j.nranges};
}

// slot bounds of one operation (also clears its workspace)
static int setop_bounds(SetopJob& j) {
    kh_ctx* c = j.c;
    if (j.empty) return KH_OK;
    c->prof_begin(KC_RANGE_BOUNDS);
    kh_launch_range_bounds(j.W, reinterpret_cast<KhSetView*>(j.d_views->p), (u32)j.in.size(), j.nranges, j.k,
                           reinterpret_cast<u64*>(j.d_bounds->p), reinterpret_cast<u64*>(j.d_lb->p),
                           j.lb_words(), c->st);
    c->prof_end();
    // Test hook (tests/test_gpu_parity.py::test_corrupt_slot_bounds_fail_closed): plant a slot bound
    // that lies past the end of operand 0, i.e. the state a broken bounds pass would leave behind.
    // The set operation must report KH_ERR_ORDER and read nothing through it.
    if (getenv("KHOICE_DEBUG_CORRUPT_BOUNDS") && j.nranges >= 2) {
        static const u64 poison = 0x0000ffffffffff00ull;
        HIPCHK(hipMemcpyAsync(reinterpret_cast<u64*>(j.d_bounds->p) + 1, &poison, 8, hipMemcpyHostToDevice, c->st));
    }
    return KH_OK;
}

// slot bounds of several planned operations (same k) in ONE launch
static int setop_bounds_batch(kh_ctx* c, std::vector<SetopJob>& jobs, Tmp& d_jobs, Pinned& pin) {
    std::vector<KhBoundsJob> hb;
    u64 max_threads = 0;
    int W = 1, k = 0;
    for (auto& j : jobs) {
        if (j.empty || j.in.empty()) continue;
        hb.push_back(setop_bounds_job(j));
        max_threads = std::max<u64>(max_threads, ((u64)j.nranges + 1) * j.in.size());
        W = j.W;
        k = j.k;
    }
    if (hb.empty()) return KH_OK;
    PIN_ALLOC(pin, sizeof(KhBoundsJob) * hb.size());
    memcpy(pin.p, hb.data(), sizeof(KhBoundsJob) * hb.size());
    TMP_ALLOC(d_jobs, c, sizeof(KhBoundsJob) * hb.size());
    HIPCHK(hipMemcpyAsync(d_jobs.b->p, pin.p, sizeof(KhBoundsJob) * hb.size(), hipMemcpyHostToDevice, c->st));
    c->prof_begin(KC_RANGE_BOUNDS);
    kh_launch_range_bounds_batch(W, d_jobs.as<KhBoundsJob>(), (u32)hb.size(), max_threads, k, c->st);
    c->prof_end();
    HIPCHK(hipGetLastError());
    return KH_OK;
}

// kernel-side description of one planned operation: one entry, or — for a histogram-only
// operation in index order — up to KH_SETOP_BATCH chains over consecutive slot ranges
static void setop_kernel_jobs(const SetopJob& j, std::vector<KhSetopJob>& out) {
    u64* desc = reinterpret_cast<u64*>(j.d_lb->p);
    u32* ctl = reinterpret_cast<u32*>(desc + j.nranges);
    u32 chains = 1;
    if (j.hist_only && !j.c->dynamic_order) chains = std::min<u32>(KH_SETOP_BATCH, std::max<u32>(1, j.nranges / 64));
    for (u32 ch = 0; ch < chains; ++ch) {
        const u32 s0 = (u32)((u64)j.nranges * ch / chains), s1 = (u32)((u64)j.nranges * (ch + 1) / chains);
        out.push_back(KhSetopJob{reinterpret_cast<const KhSetView*>(j.d_views->p),
                                 reinterpret_cast<const u64*>(j.d_bounds->p), j.okeys->p,
                                 reinterpret_cast<u32*>(j.ocnt->p), desc + s0, ctl,
                                 j.hist ? reinterpret_cast<unsigned long long*>(desc + j.nranges + 8) : nullptr,
                                 (u32)j.in.size(), j.nranges, s0, s1 - s0});
    }
}

// Planned operations of the same kind (same k, payload mode, operation, cs, hist_len) as launches
// of up to KH_SETOP_BATCH each, then the read-back of every tail.
static int setop_run_batch(kh_ctx* c, SetopJob* const* jobs, size_t njobs) {
    hipStream_t st = c->st;
    std::vector<SetopJob*> live;
    for (size_t i = 0; i < njobs; ++i)
        if (!jobs[i]->empty && !jobs[i]->in.empty()) live.push_back(jobs[i]);
    if (live.empty()) return KH_OK;
    std::vector<KhSetopJob> entries;
    const SetopJob& f = *live[0];
    for (SetopJob* jp : live) {
        const SetopJob& j = *jp;
        if (j.W != f.W || j.pay != f.pay || j.cap != f.cap || j.k != f.k || j.op != f.op || j.mode != f.mode ||
            j.cs != f.cs || j.hist_len != f.hist_len)
            return kh_fail(KH_E_INTERNAL, "set operations of different kinds in one batch");
        setop_kernel_jobs(j, entries);
    }
    for (size_t i0 = 0; i0 < entries.size(); i0 += KH_SETOP_BATCH) {
        const size_t m = std::min<size_t>(KH_SETOP_BATCH, entries.size() - i0);
        KhSetopBatch batch;
        memset(&batch, 0, sizeof batch);
        for (size_t i = 0; i < m; ++i) batch.job[i] = entries[i0 + i];
#ifdef KH_STAMPS
        Tmp d_stamps;
        u64 stamp_parts = 0;
        for (size_t i = 0; i < m; ++i) stamp_parts = std::max<u64>(stamp_parts, batch.job[i].nranges);
        stamp_parts *= m;
        TMP_ALLOC(d_stamps, c, 128 * stamp_parts);
        HIPCHK(hipMemsetAsync(d_stamps.b->p, 0, 128 * stamp_parts, st));
        kh_debug_set_stamps(d_stamps.as<u64>());
#endif
        c->prof_begin(KC_SETOP);
        kh_launch_setop(f.W, f.pay, f.cap, batch, (u32)m, f.k, f.op, f.mode, f.cs, f.hist_len, c->dynamic_order, st);
        c->prof_end();
        HIPCHK(hipGetLastError());
#ifdef KH_STAMPS
        report_stamps(c, "setop", d_stamps.b, stamp_parts);
        kh_debug_set_stamps(nullptr);
#endif
    }
    for (SetopJob* j : live)
        HIPCHK(hipMemcpyAsync(j->tail, reinterpret_cast<u64*>(j->d_lb->p) + (j->nranges - 1),
                              8 * (9 + (j->hist ? j->hist_len : 0)), hipMemcpyDeviceToHost, st));
    return KH_OK;
}

static int setop_run(SetopJob& j) {
    SetopJob* one = &j;
    return setop_run_batch(j.c, &one, 1);
}

static int setop_launch(SetopJob& j) {
    KHCHK(setop_plan(j));
    KHCHK(setop_bounds(j));
    return setop_run(j);
}

// precondition: the stream was synchronised after setop_launch(j)
static int setop_finish(SetopJob& j, kh_set** out) {
    kh_ctx* c = j.c;
    if (j.empty) {
        if (out) *out = make_set(j.k, 0, nullptr, 0, nullptr, 0, 1, j.cs);
        if (j.hist) memset(j.hist, 0, 8 * (size_t)j.hist_len);
        return KH_OK;
    }
    for (int attempt = 0; attempt < 8; ++attempt) {
        const u32 err = reinterpret_cast<const u32*>(&j.tail[1])[1];
        if (err & KH_ERR_ORDER)
            return kh_fail(KH_E_ARG, "set operation: an operand is not sorted by mixed key (kh_set_wrap_device and "
                                     "kh_set_from_device trust their caller on that); nothing was read outside it");
        if (err & KH_ERR_SPIN_TIMEOUT) {
            if (c->dynamic_order) return kh_fail(KH_E_INTERNAL, "look-back spin timed out in set operation");
            c->dynamic_order = true;      // index order did not hold: tickets from now on
            c->stat.order_fallbacks++;
            KHCHK(setop_launch(j));
            HIPCHK(hipStreamSynchronize(c->st));
            continue;
        }
        if (!(err & KH_ERR_CAPACITY)) {
            const u64 n = j.tail[3];   // outputs of all chains (control words, u64 at byte 16)
            if (out) {
                buf_ref(j.okeys);
                buf_ref(j.ocnt);
                *out = make_set(j.k, n, j.okeys, 0, j.ocnt, 0, 1, j.cs);
            }
            c->stat.setop_out += n;
            if (j.hist) memcpy(j.hist, j.pin_hist, 8 * (size_t)j.hist_len);
            return KH_OK;
        }
        c->stat.retries++;
        // the kernel recorded its fullest slot: shrink the mean fill so that one fits with 10 %
        // to spare (never by less than 1/8, by 4 when the record is missing)
        const u64 fullest = (u32)j.tail[2];
        u64 next = fullest > j.cap ? j.target * j.cap * 9 / (fullest * 10) : j.target / 4;
        // that rule assumes keys spread evenly over the ranges; operands that crowd more keys than a slot holds into
        // a sliver of the key space barely shrink under it, so from the third re-plan on the fill is quartered
        if (attempt >= 2) next = std::min<u64>(next, j.target / 4);
        // (no floor of 16 here: a few thousand keys in a thousandth of the key space need more ranges than total / 16)
        j.target = std::max<u64>(1, std::min<u64>(next, j.target * 7 / 8));
        KHCHK(setop_launch(j));
        HIPCHK(hipStreamSynchronize(c->st));
    }
    return kh_fail(KH_E_CAPACITY, "set operation: a key range still overflows LDS after 8 re-plans");
}

static int run_setop(kh_ctx* c, const std::vector<const kh_set*>& in, int op, int mode, u32 cs,
                     kh_set** out, uint64_t* hist, u32 hist_len) {
    SetopJob j;
    j.c = c; j.in = in; j.op = op; j.mode = mode; j.cs = cs; j.hist = hist; j.hist_len = hist_len;
    j.hist_only = out == nullptr;   // no set wanted: the output need not be one compact array
    KHCHK(setop_prepare(j));
    KHCHK(setop_launch(j));
    HIPCHK(hipStreamSynchronize(c->st));
    return setop_finish(j, out);
}

extern "C" int kh_union_sum(kh_ctx* c, const kh_set* const* sets, int nsets, uint32_t cs, kh_set** out,
                            uint64_t* hist, uint32_t hist_len) {
    if (!c || !sets || !out || nsets <= 0) return kh_fail(KH_E_ARG, "kh_union_sum: bad argument");
    if (hist && hist_len < 2) return kh_fail(KH_E_ARG, "hist_len must be >= 2");
    if (cs < 1) return kh_fail(KH_E_ARG, "cs must be >= 1");
    HIPCHK(hipSetDevice(c->dev));
    for (int i = 0; i < nsets; ++i)
        if (!sets[i]) return kh_fail(KH_E_ARG, "kh_union_sum: operand %d is NULL", i);
    if (nsets <= KH_MAX_INPUT_SETS) {
        std::vector<const kh_set*> in(sets, sets + nsets);
        return run_setop(c, in, KH_OP_UNION, KH_OC_SUM, cs, out, hist, hist_len);
    }
    // fan-in above one launch's limit: sum groups of up to KH_MAX_INPUT_SETS, then sum the sums.
    // The partial sums saturate at cs already: exact, since counters are never negative.
    std::vector<kh_set*> partial;
    auto cleanup = [&]() { for (auto* p : partial) kh_set_free(p); };
    for (int i = 0; i < nsets; i += KH_MAX_INPUT_SETS) {
        const int m = std::min(KH_MAX_INPUT_SETS, nsets - i);
        std::vector<const kh_set*> in(sets + i, sets + i + m);
        kh_set* p = nullptr;
        int r = run_setop(c, in, KH_OP_UNION, KH_OC_SUM, cs, &p, nullptr, 0);
        if (r != KH_OK) { cleanup(); return r; }
        partial.push_back(p);
    }
    int r = kh_union_sum(c, partial.data(), (int)partial.size(), cs, out, hist, hist_len);
    cleanup();
    return r;
}

// The histogram of a union-sum without handing the union back (steps 7+8 of experiment type 1
// when only step_8's histogram is wanted, and the merged slices of the multi-GPU exchange):
// every output record is still written, but not as one compact array, so the slots run as
// independent chains.
extern "C" int kh_union_histogram(kh_ctx* c, const kh_set* const* sets, int nsets, uint32_t cs,
                                  uint64_t* hist, uint32_t hist_len) {
    if (!c || !sets || !hist || nsets <= 0) return kh_fail(KH_E_ARG, "kh_union_histogram: bad argument");
    if (hist_len < 2) return kh_fail(KH_E_ARG, "hist_len must be >= 2");
    if (cs < 1) return kh_fail(KH_E_ARG, "cs must be >= 1");
    HIPCHK(hipSetDevice(c->dev));
    for (int i = 0; i < nsets; ++i)
        if (!sets[i]) return kh_fail(KH_E_ARG, "kh_union_histogram: operand %d is NULL", i);
    if (nsets > KH_MAX_INPUT_SETS) {   // beyond one launch's fan-in: through the general path
        kh_set* u = nullptr;
        KHCHK(kh_union_sum(c, sets, nsets, cs, &u, hist, hist_len));
        kh_set_free(u);
        return KH_OK;
    }
    std::vector<const kh_set*> in(sets, sets + nsets);
    return run_setop(c, in, KH_OP_UNION, KH_OC_SUM, cs, nullptr, hist, hist_len);
}

extern "C" int kh_simple(kh_ctx* c, const kh_set* a, const kh_set* b, int op, int mode, uint32_t cs,
                         kh_set** out) {
    if (!c || !a || !b || !out) return kh_fail(KH_E_ARG, "kh_simple: NULL argument");
    if (op < KH_UNION || op > KH_COUNTERS_SUBTRACT) return kh_fail(KH_E_ARG, "unknown set operation %d", op);
    if (mode < KH_MODE_MIN || mode > KH_MODE_RIGHT) return kh_fail(KH_E_ARG, "unknown counter mode %d", mode);
    if (cs < 1) return kh_fail(KH_E_ARG, "cs must be >= 1");
    HIPCHK(hipSetDevice(c->dev));
    std::vector<const kh_set*> in{a, b};
    return run_setop(c, in, op, mode, cs, out, nullptr, 0);
}

// ------------------------------------------------------------------------------ histogram
extern "C" int kh_histogram(kh_ctx* c, const kh_set* s, uint64_t* hist, uint32_t hist_len) {
    if (!c || !s || !hist || hist_len < 2) return kh_fail(KH_E_ARG, "kh_histogram: bad argument");
    HIPCHK(hipSetDevice(c->dev));
    memset(hist, 0, 8 * (size_t)hist_len);
    if (!s->n) return KH_OK;
    if (!s->cb) {
        hist[std::min<u32>(s->uniform, hist_len - 1)] = s->n;
        return KH_OK;
    }
    Tmp d_hist;
    TMP_ALLOC(d_hist, c, 8 * (u64)hist_len);
    HIPCHK(hipMemsetAsync(d_hist.b->p, 0, 8 * (u64)hist_len, c->st));
    c->prof_begin(KC_HISTOGRAM);
    kh_launch_histogram(s->counts_ptr(), s->n, d_hist.as<unsigned long long>(), hist_len, c->st);
    c->prof_end();
    HIPCHK(hipMemcpyAsync(hist, d_hist.b->p, 8 * (size_t)hist_len, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return KH_OK;
}

// ------------------------------------------------------------------- occurrence table
// Small-k variant of the across-group step: cell v of a 4^k-cell table in
// device memory counts the sets that hold canonical k-mer v.
extern "C" int kh_table_add_set(kh_ctx* c, const kh_set* s, void* d_table, uint32_t cell_bytes) {
    if (!c || !s || !d_table) return kh_fail(KH_E_ARG, "kh_table_add_set: NULL argument");
    if (cell_bytes != 1 && cell_bytes != 4) return kh_fail(KH_E_ARG, "kh_table_add_set: cell_bytes must be 1 or 4");
    if (s->k > KH_TABLE_MAX_K) return kh_fail(KH_E_ARG, "kh_table_add_set: k > 16 has no direct-addressed table");
    HIPCHK(hipSetDevice(c->dev));
    if (!s->n) return KH_OK;
    c->prof_begin(KC_HISTOGRAM);
    kh_launch_table_add(s->keys_ptr(), s->n, s->k, d_table, cell_bytes, c->st);
    c->prof_end();
    HIPCHK(hipGetLastError());
    return KH_OK;
}

extern "C" int kh_table_histogram(kh_ctx* c, const void* d_table, uint32_t cell_bytes, uint64_t lo,
                                  uint64_t hi, uint32_t cs, uint64_t* hist, uint32_t hist_len) {
    if (!c || !d_table || !hist || hist_len < 2) return kh_fail(KH_E_ARG, "kh_table_histogram: bad argument");
    if (cell_bytes != 1 && cell_bytes != 4) return kh_fail(KH_E_ARG, "kh_table_histogram: cell_bytes must be 1 or 4");
    if (hi < lo || (lo * cell_bytes) % 16 || ((uintptr_t)d_table % 16))
        return kh_fail(KH_E_ARG, "kh_table_histogram: the range must start on a 16-byte boundary");
    HIPCHK(hipSetDevice(c->dev));
    memset(hist, 0, 8 * (size_t)hist_len);
    if (hi == lo) return KH_OK;
    Tmp d_hist;
    TMP_ALLOC(d_hist, c, 8 * (u64)hist_len);
    HIPCHK(hipMemsetAsync(d_hist.b->p, 0, 8 * (u64)hist_len, c->st));
    c->prof_begin(KC_HISTOGRAM);
    kh_launch_table_hist(d_table, cell_bytes, lo, hi, cs ? cs : 0xFFFFFFFFu, d_hist.as<unsigned long long>(),
                         hist_len, c->st);
    c->prof_end();
    HIPCHK(hipMemcpyAsync(hist, d_hist.b->p, 8 * (size_t)hist_len, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return KH_OK;
}

// ------------------------------------------------------------------- membership matrix
// Experiment type 4 (src/merge_lists.py:14-33,101-141): which of `sets` hold each pivot k-mer.
// Device: one search per (pivot key, set).  Host: the records are put in the order the
// reference walks them — its dict is filled from the `dump -s` text, i.e. ascending canonical
// key — because the floating-point row sums below depend on the order of the additions.
namespace {
struct KeyIdx { u64 key; u32 idx; };

// ascending order of n canonical keys; W == 1: LSD radix over the 2k significant bits
void canonical_order(int W, int k, const u64* keys, u64 n, std::vector<u32>& order) {
    order.resize(n);
    if (W == 2) {
        for (u64 i = 0; i < n; ++i) order[i] = (u32)i;
        std::sort(order.begin(), order.end(), [&](u32 a, u32 b) {
            return keys[2 * (u64)a + 1] != keys[2 * (u64)b + 1] ? keys[2 * (u64)a + 1] < keys[2 * (u64)b + 1]
                                                                : keys[2 * (u64)a] < keys[2 * (u64)b];
        });
        return;
    }
    std::vector<KeyIdx> a(n), b(n);
    for (u64 i = 0; i < n; ++i) a[i] = KeyIdx{keys[i], (u32)i};
    const int bits = 2 * k;
    for (int sh = 0; sh < bits; sh += 11) {
        size_t cnt[2049] = {0};
        for (u64 i = 0; i < n; ++i) ++cnt[((a[i].key >> sh) & 2047) + 1];
        for (int d = 0; d < 2048; ++d) cnt[d + 1] += cnt[d];
        for (u64 i = 0; i < n; ++i) b[cnt[(a[i].key >> sh) & 2047]++] = a[i];
        a.swap(b);
    }
    for (u64 i = 0; i < n; ++i) order[i] = a[i].idx;
}

struct Membership {
    std::vector<u64> keys;     // canonical, as stored (mixed order)
    std::vector<u32> counts;
    std::vector<u64> masks;
    std::vector<u32> order;    // ascending canonical key
    u32 nwords = 0;
};

int membership_compute(kh_ctx* c, const kh_set* pivot, const kh_set* const* sets, int nsets, Membership& m) {
    if (!c || !pivot || (nsets > 0 && !sets) || nsets < 0) return kh_fail(KH_E_ARG, "membership: bad argument");
    if (pivot->n >> 32) return kh_fail(KH_E_ARG, "membership: pivot sets of 2^32 k-mers or more are not supported");
    for (int i = 0; i < nsets; ++i) {
        if (!sets[i]) return kh_fail(KH_E_ARG, "membership: NULL set");
        if (sets[i]->k != pivot->k) return kh_fail(KH_E_KMISMATCH, "membership: k differs (%d vs %d)", sets[i]->k, pivot->k);
    }
    HIPCHK(hipSetDevice(c->dev));
    const u64 n = pivot->n;
    const int W = pivot->W;
    m.nwords = (u32)std::max(1, (nsets + 63) / 64);
    m.keys.assign(n * W, 0);
    m.counts.assign(n, pivot->uniform);
    m.masks.assign(n * m.nwords, 0);
    if (!n) { m.order.clear(); return KH_OK; }
    std::vector<KhSetView> v((size_t)std::max(nsets, 1));
    for (int i = 0; i < nsets; ++i)
        v[i] = KhSetView{sets[i]->n ? sets[i]->keys_ptr() : nullptr, nullptr, sets[i]->n, 1, 0};
    Tmp d_view, d_masks, d_keys;
    TMP_ALLOC(d_view, c, sizeof(KhSetView) * v.size());
    TMP_ALLOC(d_masks, c, 8 * n * m.nwords);
    TMP_ALLOC(d_keys, c, 8 * (u64)W * n);
    HIPCHK(hipMemcpyAsync(d_view.b->p, v.data(), sizeof(KhSetView) * v.size(), hipMemcpyHostToDevice, c->st));
    c->prof_begin(KC_SETOP);
    kh_launch_membership(W, pivot->keys_ptr(), n, d_view.as<KhSetView>(), (u32)nsets, pivot->k, m.nwords,
                         d_masks.as<u64>(), c->st);
    c->prof_end();
    kh_launch_unmix(W, pivot->keys_ptr(), d_keys.b->p, n, pivot->k, c->st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(m.masks.data(), d_masks.b->p, 8 * n * m.nwords, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(m.keys.data(), d_keys.b->p, 8 * (u64)W * n, hipMemcpyDeviceToHost, c->st));
    if (pivot->cb)
        HIPCHK(hipMemcpyAsync(m.counts.data(), pivot->counts_ptr(), 4 * n, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    canonical_order(W, pivot->k, m.keys.data(), n, m.order);
    return KH_OK;
}
}  // namespace

extern "C" int kh_membership(kh_ctx* c, const kh_set* pivot, const kh_set* const* sets, int nsets,
                             uint64_t* keys_out, uint32_t* counts_out, uint64_t* masks_out) {
    Membership m;
    KHCHK(membership_compute(c, pivot, sets, nsets, m));
    const int W = pivot->W;
    for (u64 r = 0; r < pivot->n; ++r) {
        const u64 i = m.order[r];
        if (keys_out) for (int w = 0; w < W; ++w) keys_out[r * W + w] = m.keys[i * W + w];
        if (counts_out) counts_out[r] = m.counts[i];
        if (masks_out) for (u32 w = 0; w < m.nwords; ++w) masks_out[r * m.nwords + w] = m.masks[i * m.nwords + w];
    }
    return KH_OK;
}

// One row of the feature-level confusion matrix, exactly as src/merge_lists.py:122-141 adds it
// up: k-mers in dump order; for a k-mer with count c held by the sets M (ascending index, the
// order update_dictionary appends them, :26-33), row[m] += 1 / len(M) * c for m in M;
// unique_pivot_count = sum of c over the k-mers no set holds (:122-126).
// The sum itself, shared by kh_confusion_row and kh_exp4_run: record r (ascending canonical key) is masks[i * nwords ..]
// and counts[i] with i = order ? order[r] : r.  One rounding per operation, no contraction, every partial sum stored.
static void confusion_sum(const u64* masks, const u32* counts, const u32* order, u64 n, u32 nwords, int nsets,
                          double* row, uint64_t* unique_pivot_count) {
#pragma clang fp contract(off)
    for (int d = 0; d < nsets; ++d) row[d] = 0.0;
    u64 uniq = 0;
    for (u64 r = 0; r < n; ++r) {
        const u64 i = order ? order[r] : r;
        int len = 0;
        for (u32 w = 0; w < nwords; ++w) len += __builtin_popcountll(masks[i * nwords + w]);
        if (!len) { uniq += counts[i]; continue; }
        const double share = 1.0 / (double)len;              // Python: 1 / len(matches)
        const double add = share * (double)counts[i];        //         ... * count
        for (u32 w = 0; w < nwords; ++w) {
            u64 bits = masks[i * nwords + w];
            while (bits) {
                const int d = __builtin_ctzll(bits);
                bits &= bits - 1;
                volatile double sum = row[w * 64 + d] + add;
                row[w * 64 + d] = sum;
            }
        }
    }
    *unique_pivot_count = uniq;
}
extern "C" int kh_confusion_row(kh_ctx* c, const kh_set* pivot, const kh_set* const* sets, int nsets,
                                double* row, uint64_t* unique_pivot_count) {
    if (!row || !unique_pivot_count) return kh_fail(KH_E_ARG, "kh_confusion_row: NULL output");
    Membership m;
    KHCHK(membership_compute(c, pivot, sets, nsets, m));
    confusion_sum(m.masks.data(), m.counts.data(), m.order.data(), pivot->n, m.nwords, nsets, row, unique_pivot_count);
    return KH_OK;
}

// ------------------------------------------------------------------- read-level votes
// Experiment type 6 (src/merge_lists.py:151-183): per read the votes, the k-mers no set holds and the sets that tie
// for the highest vote; the draw among them (:180) stays with the caller.  Device: k_read_masks, k_read_fold
// (kh_reads.hip).  The mask buffer costs 8 * nwords bytes per text position: a quarter of the free HBM is its budget,
// and a text above it runs as batches of whole reads (KHOICE_READS_MAX_POS lowers the budget, in positions).
static u64 reads_max_pos(kh_ctx* c, u32 nwords) {
    u64 budget = 1ull << 30;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = (free_b + c->pool.cached_bytes) / 4;
    u64 pos = std::max<u64>(1, budget / (8ull * nwords + 1));
    if (const char* e = getenv("KHOICE_READS_MAX_POS")) pos = std::min(pos, std::max<u64>(1, strtoull(e, nullptr, 10)));
    return pos;
}
// What both forms of the votes do alike, from the layout checks of the reads to the read-back: the batches of whole
// reads, every batch's text, offsets and control words uploaded, its masks, the fold, its outputs and the two errors.
// mask_launch(job) queues the kernel that fills job.masks (k_read_masks against sorted sets, which also sets job.sets
// and job.check; k_read_lookup against a mask table) and returns a status.
template <class F>
static int read_votes_batches(kh_ctx* c, const uint8_t* reads, const uint64_t* read_off, uint64_t nreads, int on_device, int k, int nsets,
                              uint64_t* tie_masks, double* votes, uint32_t* unmatched, F mask_launch) {
    if (!nreads) return KH_OK;
    if (!reads || !tie_masks) return kh_fail(KH_E_ARG, "kh_read_votes: NULL argument");
    if (nreads >= 0xffffffffull) return kh_fail(KH_E_ARG, "kh_read_votes: 2^32 - 1 reads or more are not supported");
    for (u64 i = 0; i < nreads; ++i) {
        if (read_off[i + 1] <= read_off[i])
            return kh_fail(KH_E_ARG, "kh_read_votes: read_off[%llu] leaves no room for read %llu and its newline",
                           (unsigned long long)(i + 1), (unsigned long long)i);
        if (on_device) continue;   // (a device text is the caller's word)
        const u8* b = reads + read_off[i];
        const u64 len = read_off[i + 1] - 1 - read_off[i];
        if (b[len] != '\n' || memchr(b, '\n', len))
            return kh_fail(KH_E_ARG, "kh_read_votes: read %llu is not one line followed by a newline", (unsigned long long)i);
    }
    HIPCHK(hipSetDevice(c->dev));
    const u32 nwords = (u32)((nsets + 63) / 64);
    std::vector<double> inv(64 * (size_t)nwords + 1, 0.0);
    for (size_t L = 1; L < inv.size(); ++L) inv[L] = 1.0 / (double)L;     // Python: 1 / len(matches)
    Tmp d_inv;
    TMP_ALLOC(d_inv, c, 8 * inv.size());
    HIPCHK(hipMemcpyAsync(d_inv.b->p, inv.data(), 8 * inv.size(), hipMemcpyHostToDevice, c->st));
    const u64 max_pos = reads_max_pos(c, nwords);
    std::vector<u64> rel;
    for (u64 b0 = 0; b0 < nreads;) {
        u64 b1 = b0 + 1;                                                   // a batch holds at least one read
        while (b1 < nreads && read_off[b1 + 1] - read_off[b0] <= max_pos) ++b1;
        const u64 nb = b1 - b0, npos = read_off[b1] - read_off[b0];
        rel.resize(nb + 1);
        for (u64 i = 0; i <= nb; ++i) rel[i] = read_off[b0 + i] - read_off[b0];
        const u32 ctl0[4] = {0, 0xffffffffu, 0xffffffffu, 0};
        u32 ctl[4];
        Tmp d_text, d_off, d_masks, d_tie, d_votes, d_unm, d_ctl;
        TMP_ALLOC(d_off, c, 8 * (nb + 1));
        TMP_ALLOC(d_masks, c, 8 * (u64)nwords * npos);
        TMP_ALLOC(d_tie, c, 8 * (u64)nwords * nb);
        TMP_ALLOC(d_ctl, c, sizeof ctl0);
        if (votes) TMP_ALLOC(d_votes, c, 8 * (u64)nsets * nb);
        if (unmatched) TMP_ALLOC(d_unm, c, 4 * nb);
        const u8* text = reads + read_off[b0];
        if (!on_device) {
            TMP_ALLOC(d_text, c, npos);
            HIPCHK(hipMemcpyAsync(d_text.b->p, text, npos, hipMemcpyHostToDevice, c->st));
            text = d_text.as<u8>();
        }
        HIPCHK(hipMemcpyAsync(d_off.b->p, rel.data(), 8 * (nb + 1), hipMemcpyHostToDevice, c->st));
        HIPCHK(hipMemcpyAsync(d_ctl.b->p, ctl0, sizeof ctl0, hipMemcpyHostToDevice, c->st));
        KhReadsJob job{text, npos, d_off.as<u64>(), (u32)nb, (u32)b0, nullptr, nullptr, (u32)nsets, nwords, k, d_masks.as<u64>(),
                       d_ctl.as<u32>()};
        KHCHK(mask_launch(job));
        const u32 grid = (u32)std::min<u64>((nb + 3) / 4, (u64)std::max(1, c->cus) * 8);
        c->prof_begin(KC_READ_FOLD);
        kh_launch_read_fold(job, d_inv.as<double>(), d_tie.as<u64>(), votes ? d_votes.as<double>() : nullptr,
                            unmatched ? d_unm.as<u32>() : nullptr, grid, c->st);
        c->prof_end();
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(ctl, d_ctl.b->p, sizeof ctl, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipMemcpyAsync(tie_masks + b0 * nwords, d_tie.b->p, 8 * (u64)nwords * nb, hipMemcpyDeviceToHost, c->st));
        if (votes) HIPCHK(hipMemcpyAsync(votes + b0 * (u64)nsets, d_votes.b->p, 8 * (u64)nsets * nb, hipMemcpyDeviceToHost, c->st));
        if (unmatched) HIPCHK(hipMemcpyAsync(unmatched + b0, d_unm.b->p, 4 * nb, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
        // reads are batched in order, so the first batch with an error holds the lowest such read
        if (ctl[1] <= ctl[2] && ctl[1] != 0xffffffffu)
            return kh_fail(KH_E_ARG, "kh_read_votes: read %u holds a byte outside upper-case ACGT (src/merge_lists.py:66)", ctl[1]);
        if (ctl[2] != 0xffffffffu)
            return kh_fail(KH_E_ARG, "kh_read_votes: read %u has a k-mer that the check set does not hold (src/merge_lists.py:167)", ctl[2]);
        b0 = b1;
    }
    return KH_OK;
}
extern "C" int kh_read_votes(kh_ctx* c, const uint8_t* reads, const uint64_t* read_off, uint64_t nreads, int on_device,
                             int k, const kh_set* const* sets, int nsets, const kh_set* check, uint64_t* tie_masks,
                             double* votes, uint32_t* unmatched) {
    if (!c || !read_off) return kh_fail(KH_E_ARG, "kh_read_votes: NULL argument");
    if (nsets < 1 || !sets) return kh_fail(KH_E_ARG, "kh_read_votes: at least one set is needed (nsets = %d)", nsets);
    if ((u32)nsets > KH_READS_MAX_SETS)
        return kh_fail(KH_E_ARG, "kh_read_votes: more than %u sets are not supported", KH_READS_MAX_SETS);
    KHCHK(check_k(k));
    for (int i = 0; i < nsets; ++i) {
        if (!sets[i]) return kh_fail(KH_E_ARG, "kh_read_votes: NULL set");
        if (sets[i]->k != k) return kh_fail(KH_E_KMISMATCH, "kh_read_votes: k differs (set %d has %d, asked %d)", i, sets[i]->k, k);
    }
    if (check && check->k != k) return kh_fail(KH_E_KMISMATCH, "kh_read_votes: k differs (check set has %d, asked %d)", check->k, k);
    const int W = k <= 32 ? 1 : 2;
    std::vector<KhSetView> v;     // the sets' views, then the check set's: uploaded in front of the first batch's masks
    Tmp d_view;
    return read_votes_batches(c, reads, read_off, nreads, on_device, k, nsets, tie_masks, votes, unmatched, [&](KhReadsJob& job) {
        if (!d_view.b) {
            v.resize((size_t)nsets + 1);
            for (int i = 0; i < nsets; ++i) v[i] = KhSetView{sets[i]->n ? sets[i]->keys_ptr() : nullptr, nullptr, sets[i]->n, 1, 0};
            v[nsets] = check ? KhSetView{check->n ? check->keys_ptr() : nullptr, nullptr, check->n, 1, 0} : KhSetView{nullptr, nullptr, 0, 1, 0};
            TMP_ALLOC(d_view, c, sizeof(KhSetView) * v.size());
            HIPCHK(hipMemcpyAsync(d_view.b->p, v.data(), sizeof(KhSetView) * v.size(), hipMemcpyHostToDevice, c->st));
        }
        job.sets = d_view.as<KhSetView>();
        job.check = check ? d_view.as<KhSetView>() + nsets : nullptr;
        c->prof_begin(KC_READ_MASKS);
        kh_launch_read_masks(W, job, c->st);
        c->prof_end();
        return (int)KH_OK;
    });
}

// ------------------------------------------------------------------- merged mask index
// The union of nsets sets with a mask per key and a bucket directory in front (kh_index.hip): one lookup
// per key whatever nsets is.  Built from sorted sets by the n-ary union (the keys), k_index_dir (the directory) and
// k_index_tag (the masks); the index owns all three arrays and keeps no reference to the sets.
constexpr u64 KH_INDEX_BUCKET_KEYS = 4;   // B: keys per bucket of the directory (KHOICE_INDEX_BUCKET_KEYS overrides it, per build)
static u64 index_bucket_keys() {
    u64 b = KH_INDEX_BUCKET_KEYS;
    if (const char* e = getenv("KHOICE_INDEX_BUCKET_KEYS")) b = std::max<u64>(1, strtoull(e, nullptr, 10));
    return b;
}
static u32 index_buckets(u64 n, u64 bucket_keys) {
    return (u32)std::min<u64>(1ull << 31, std::max<u64>(1, (n + bucket_keys - 1) / bucket_keys));
}
static KhIndexView index_view(const kh_index* ix) {
    return KhIndexView{ix->n ? ix->keys->keys_ptr() : nullptr, reinterpret_cast<const u64*>(ix->masks->p),
                       reinterpret_cast<const u64*>(ix->dir->p), ix->n, ix->nb, ix->mwords};
}
extern "C" void kh_index_free(kh_index* ix) {
    if (!ix) return;
    kh_set_free(ix->keys);
    buf_unref(ix->masks);
    buf_unref(ix->dir);
    delete ix;
}
extern "C" int kh_index_build(kh_ctx* c, const kh_set* const* sets, int nsets, kh_index** out) {
    if (!c || !out) return kh_fail(KH_E_ARG, "kh_index_build: NULL argument");
    if (nsets < 1 || !sets) return kh_fail(KH_E_ARG, "kh_index_build: at least one set is needed (nsets = %d)", nsets);
    if ((u32)nsets > KH_READS_MAX_SETS)
        return kh_fail(KH_E_ARG, "kh_index_build: more than %u sets are not supported", KH_READS_MAX_SETS);
    for (int i = 0; i < nsets; ++i) {
        if (!sets[i]) return kh_fail(KH_E_ARG, "kh_index_build: NULL set");
        if (sets[i]->k != sets[0]->k)
            return kh_fail(KH_E_KMISMATCH, "kh_index_build: k differs (set %d has %d, asked %d)", i, sets[i]->k, sets[0]->k);
    }
    HIPCHK(hipSetDevice(c->dev));
    struct Guard { kh_index* ix; ~Guard() { kh_index_free(ix); } } g{new kh_index{}};
    kh_index* ix = g.ix;
    ix->k = sets[0]->k;
    ix->W = sets[0]->W;
    ix->nsets = nsets;
    ix->mwords = (u32)std::max(1, (nsets + 63) / 64);
    u64 max_n = 0;
    for (int i = 0; i < nsets; ++i) max_n = std::max<u64>(max_n, sets[i]->n);
    {   // the keys: the existing n-ary union; its counters are dropped at once
        kh_set* u = nullptr;
        KHCHK(kh_union_sum(c, sets, nsets, 1, &u, nullptr, 0));
        const int r = kh_set_counts(c, u, 1, &ix->keys);
        kh_set_free(u);
        KHCHK(r);
    }
    ix->n = ix->keys->n;
    ix->nb = index_buckets(ix->n, index_bucket_keys());
    ix->masks = c->buf_alloc(8 * ix->n * ix->mwords);
    ix->dir = c->buf_alloc(8 * ((u64)ix->nb + 1));
    if (!ix->masks || !ix->dir)
        return kh_fail(KH_E_NOMEM, "kh_index_build: the index of %llu keys, %u mask words and %u buckets does not fit",
                       (unsigned long long)ix->n, ix->mwords, ix->nb);
    const KhIndexView v = index_view(ix);
    c->prof_begin(KC_INDEX_DIR);
    kh_launch_index_dir(ix->W, v, reinterpret_cast<u64*>(ix->dir->p), ix->k, c->st);
    c->prof_end();
    HIPCHK(hipGetLastError());
    if (ix->n) {
        std::vector<KhSetView> sv((size_t)nsets);
        for (int i = 0; i < nsets; ++i) sv[i] = KhSetView{sets[i]->n ? sets[i]->keys_ptr() : nullptr, nullptr, sets[i]->n, 1, 0};
        Tmp d_view, d_err;
        TMP_ALLOC(d_view, c, sizeof(KhSetView) * sv.size());
        TMP_ALLOC(d_err, c, 4);
        HIPCHK(hipMemcpyAsync(d_view.b->p, sv.data(), sizeof(KhSetView) * sv.size(), hipMemcpyHostToDevice, c->st));
        HIPCHK(hipMemsetAsync(d_err.b->p, 0, 4, c->st));
        HIPCHK(hipMemsetAsync(ix->masks->p, 0, 8 * ix->n * ix->mwords, c->st));   // k_index_tag ORs into zeros
        c->prof_begin(KC_INDEX_TAG);
        kh_launch_index_tag(ix->W, v, reinterpret_cast<u64*>(ix->masks->p), d_view.as<KhSetView>(), (u32)nsets, max_n, ix->k,
                            d_err.as<u32>(), c->st);
        c->prof_end();
        HIPCHK(hipGetLastError());
        u32 err = 0;
        HIPCHK(hipMemcpyAsync(&err, d_err.b->p, 4, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
        if (err) return kh_fail(KH_E_INTERNAL, "kh_index_build: a key of a set is missing from the union of the sets");
    } else {
        HIPCHK(hipStreamSynchronize(c->st));
    }
    *out = ix;
    g.ix = nullptr;
    return KH_OK;
}
extern "C" int kh_index_info(const kh_index* ix, uint64_t* n, int* k, int* nsets, int* mask_words, uint64_t* nbuckets) {
    if (!ix) return kh_fail(KH_E_ARG, "index is NULL");
    if (n) *n = ix->n;
    if (k) *k = ix->k;
    if (nsets) *nsets = ix->nsets;
    if (mask_words) *mask_words = (int)ix->mwords;
    if (nbuckets) *nbuckets = ix->nb;
    return KH_OK;
}
extern "C" int kh_index_download(kh_ctx* c, const kh_index* ix, uint64_t* keys, uint64_t* masks) {
    if (!c || !ix) return kh_fail(KH_E_ARG, "kh_index_download: NULL argument");
    if (keys) KHCHK(kh_set_download(c, ix->keys, keys, nullptr));
    if (masks && ix->n) {
        HIPCHK(hipSetDevice(c->dev));
        HIPCHK(hipMemcpyAsync(masks, ix->masks->p, 8 * ix->n * ix->mwords, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
    }
    return KH_OK;
}
extern "C" int kh_index_masks(kh_ctx* c, const kh_index* ix, const kh_set* probe, uint64_t* masks_out) {
    if (!c || !ix || !probe) return kh_fail(KH_E_ARG, "kh_index_masks: NULL argument");
    if (probe->k != ix->k) return kh_fail(KH_E_KMISMATCH, "kh_index_masks: k differs (probe has %d, the index %d)", probe->k, ix->k);
    if (!probe->n) return KH_OK;
    if (!masks_out) return kh_fail(KH_E_ARG, "kh_index_masks: NULL argument");
    HIPCHK(hipSetDevice(c->dev));
    Tmp d_out;
    TMP_ALLOC(d_out, c, 8 * probe->n * ix->mwords);
    c->prof_begin(KC_INDEX_MEMBER);
    kh_launch_index_member(ix->W, index_view(ix), probe->keys_ptr(), probe->n, ix->k, d_out.as<u64>(), c->st);
    c->prof_end();
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(masks_out, d_out.b->p, 8 * probe->n * ix->mwords, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return KH_OK;
}
// The votes of read_votes_batches with the masks from an index: what kh_read_votes_index and exp6_index share.
static int read_votes_index(kh_ctx* c, const uint8_t* reads, const uint64_t* read_off, uint64_t nreads, int on_device,
                            const kh_index* ix, const kh_set* check, uint64_t* tie_masks, double* votes, uint32_t* unmatched) {
    const KhIndexView v = index_view(ix);
    Tmp d_check;
    return read_votes_batches(c, reads, read_off, nreads, on_device, ix->k, ix->nsets, tie_masks, votes, unmatched, [&](KhReadsJob& job) {
        if (check && !d_check.b) {
            const KhSetView cv{check->n ? check->keys_ptr() : nullptr, nullptr, check->n, 1, 0};
            TMP_ALLOC(d_check, c, sizeof cv);
            HIPCHK(hipMemcpyAsync(d_check.b->p, &cv, sizeof cv, hipMemcpyHostToDevice, c->st));
        }
        job.check = check ? d_check.as<KhSetView>() : nullptr;
        c->prof_begin(KC_READ_INDEX);
        kh_launch_read_index(ix->W, job, v, c->st);
        c->prof_end();
        return (int)KH_OK;
    });
}
extern "C" int kh_read_votes_index(kh_ctx* c, const uint8_t* reads, const uint64_t* read_off, uint64_t nreads, int on_device,
                                   const kh_index* ix, const kh_set* check, uint64_t* tie_masks, double* votes,
                                   uint32_t* unmatched) {
    if (!c || !read_off || !ix) return kh_fail(KH_E_ARG, "kh_read_votes_index: NULL argument");
    if (check && check->k != ix->k)
        return kh_fail(KH_E_KMISMATCH, "kh_read_votes_index: k differs (check set has %d, asked %d)", check->k, ix->k);
    return read_votes_index(c, reads, read_off, nreads, on_device, ix, check, tie_masks, votes, unmatched);
}

// ------------------------------------------------------------------------------ transfer
extern "C" int kh_set_download(kh_ctx* c, const kh_set* s, uint64_t* keys, uint32_t* counts) {
    if (!c || !s) return kh_fail(KH_E_ARG, "kh_set_download: NULL argument");
    HIPCHK(hipSetDevice(c->dev));
    if (!s->n) return KH_OK;
    const size_t kb = 8 * (size_t)s->W;
    if (keys) {
        Tmp d_tmp;
        TMP_ALLOC(d_tmp, c, kb * s->n);
        c->prof_begin(KC_REMIX);
        kh_launch_unmix(s->W, s->keys_ptr(), d_tmp.b->p, s->n, s->k, c->st);
        c->prof_end();
        HIPCHK(hipMemcpyAsync(keys, d_tmp.b->p, kb * s->n, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
    }
    if (counts) {
        if (s->cb) {
            HIPCHK(hipMemcpyAsync(counts, s->counts_ptr(), 4 * s->n, hipMemcpyDeviceToHost, c->st));
            HIPCHK(hipStreamSynchronize(c->st));
        } else {
            std::fill(counts, counts + s->n, s->uniform);
        }
    }
    return KH_OK;
}

int kh_set_from_mixed_host(kh_ctx* c, int k, u64 n, const void* keys_mixed_sorted, const u32* counts,
                           u32 uniform, u32 counter_max, kh_set** out) {
    const int W = k <= 32 ? 1 : 2;
    const size_t kb = 8 * (size_t)W;
    if (!n) { *out = make_set(k, 0, nullptr, 0, nullptr, 0, uniform, counter_max); return KH_OK; }
    DevBuf* kbuf = c->buf_alloc(kb * n);
    DevBuf* cbuf = counts ? c->buf_alloc(4 * n) : nullptr;
    struct Guard { DevBuf *a, *b; ~Guard() { buf_unref(a); buf_unref(b); } } guard{kbuf, cbuf};
    if (!kbuf || (counts && !cbuf)) return kh_fail(KH_E_NOMEM, "device allocation failed (upload)");
    HIPCHK(hipMemcpyAsync(kbuf->p, keys_mixed_sorted, kb * n, hipMemcpyHostToDevice, c->st));
    if (counts) HIPCHK(hipMemcpyAsync(cbuf->p, counts, 4 * n, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    buf_ref(kbuf);
    if (cbuf) buf_ref(cbuf);
    *out = make_set(k, n, kbuf, 0, cbuf, 0, uniform, counter_max);
    return KH_OK;
}

extern "C" int kh_set_upload(kh_ctx* c, int k, uint64_t n, const uint64_t* keys, const uint32_t* counts,
                             kh_set** out) {
    if (!c || !out || (n && !keys)) return kh_fail(KH_E_ARG, "kh_set_upload: bad argument");
    KHCHK(check_k(k));
    HIPCHK(hipSetDevice(c->dev));
    const int W = k <= 32 ? 1 : 2;
    // a key of 4^k or more would mix into a wrong slot and come back as another key; a zero
    // counter would be carried into unions, which never hold one
    const u64 top_mask = W == 1 ? ~kh_mask(2 * k) : ~kh_mask(2 * k - 64);
    for (u64 i = 0; i < n; ++i) {
        if (keys[i * W + W - 1] & top_mask)
            return kh_fail(KH_E_ARG, "kh_set_upload: key %llu is not below 4^%d", (unsigned long long)i, k);
        if (counts && counts[i] == 0)
            return kh_fail(KH_E_ARG, "kh_set_upload: counter %llu is 0", (unsigned long long)i);
    }
    // order by mixed key on the host (upload is a test / interchange path, not the hot path)
    std::vector<u64> mixed((size_t)n * W);
    for (u64 i = 0; i < n; ++i) kh_mix_host(k, keys + i * W, mixed.data() + i * W);
    std::vector<u64> idx(n);
    for (u64 i = 0; i < n; ++i) idx[i] = i;
    if (W == 1)
        std::sort(idx.begin(), idx.end(), [&](u64 a, u64 b) { return mixed[a] < mixed[b]; });
    else
        std::sort(idx.begin(), idx.end(), [&](u64 a, u64 b) {
            return mixed[2 * a + 1] < mixed[2 * b + 1] ||
                   (mixed[2 * a + 1] == mixed[2 * b + 1] && mixed[2 * a] < mixed[2 * b]);
        });
    std::vector<u64> sk((size_t)n * W);
    std::vector<u32> sc(counts ? n : 0);
    for (u64 i = 0; i < n; ++i) {
        for (int w = 0; w < W; ++w) sk[i * W + w] = mixed[idx[i] * W + w];
        if (counts) sc[i] = counts[idx[i]];
        if (i && memcmp(&sk[i * W], &sk[(i - 1) * W], 8 * W) == 0)
            return kh_fail(KH_E_ARG, "kh_set_upload: keys are not distinct");
    }
    return kh_set_from_mixed_host(c, k, n, sk.data(), counts ? sc.data() : nullptr, 1, KH_KMC_DEFAULT_CS, out);
}

extern "C" int kh_set_from_device(kh_ctx* c, int k, uint64_t n, const void* keys_mixed, const uint32_t* counts,
                                  kh_set** out) {
    if (!c || !out || (n && !keys_mixed)) return kh_fail(KH_E_ARG, "kh_set_from_device: bad argument");
    KHCHK(check_k(k));
    HIPCHK(hipSetDevice(c->dev));
    const int W = k <= 32 ? 1 : 2;
    const size_t kb = 8 * (size_t)W;
    if (!n) { *out = make_set(k, 0, nullptr, 0, nullptr, 0, 1); return KH_OK; }
    DevBuf* kbuf = c->buf_alloc(kb * n);
    DevBuf* cbuf = counts ? c->buf_alloc(4 * n) : nullptr;
    struct Guard { DevBuf *a, *b; ~Guard() { buf_unref(a); buf_unref(b); } } guard{kbuf, cbuf};
    if (!kbuf || (counts && !cbuf)) return kh_fail(KH_E_NOMEM, "device allocation failed");
    HIPCHK(hipMemcpyAsync(kbuf->p, keys_mixed, kb * n, hipMemcpyDeviceToDevice, c->st));
    if (counts) HIPCHK(hipMemcpyAsync(cbuf->p, counts, 4 * n, hipMemcpyDeviceToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    buf_ref(kbuf);
    if (cbuf) buf_ref(cbuf);
    *out = make_set(k, n, kbuf, 0, cbuf, 0, 1);
    return KH_OK;
}

extern "C" int kh_set_export_range(kh_ctx* c, const kh_set* s, uint64_t lo, uint64_t hi, void* keys_out,
                                   uint32_t* counts_out) {
    if (!c || !s) return kh_fail(KH_E_ARG, "kh_set_export_range: NULL argument");
    if (lo > hi || hi > s->n) return kh_fail(KH_E_ARG, "kh_set_export_range: [%llu,%llu) outside [0,%llu)",
                                             (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)s->n);
    HIPCHK(hipSetDevice(c->dev));
    const u64 n = hi - lo;
    if (!n) return KH_OK;
    const size_t kb = 8 * (size_t)s->W;
    if (keys_out)
        HIPCHK(hipMemcpyAsync(keys_out, static_cast<const u8*>(s->keys_ptr()) + lo * kb, kb * n,
                              hipMemcpyDeviceToDevice, c->st));
    if (counts_out) {
        if (s->cb) HIPCHK(hipMemcpyAsync(counts_out, s->counts_ptr() + lo, 4 * n, hipMemcpyDeviceToDevice, c->st));
        else kh_launch_fill_u32(counts_out, n, s->uniform, c->st);
    }
    return KH_OK;   // stream-ordered: call kh_sync before another stream reads the buffers
}
extern "C" int kh_set_export_device(kh_ctx* c, const kh_set* s, void* keys_out, uint32_t* counts_out) {
    if (!c || !s) return kh_fail(KH_E_ARG, "kh_set_export_device: NULL argument");
    int r = kh_set_export_range(c, s, 0, s->n, keys_out, counts_out);
    if (r != KH_OK) return r;
    HIPCHK(hipStreamSynchronize(c->st));
    return KH_OK;
}
// zero-copy view of caller-owned device arrays (mixed keys ascending, distinct); the caller
// keeps them alive and unchanged for the life of the handle
extern "C" int kh_set_wrap_device(kh_ctx* c, int k, uint64_t n, const void* keys_mixed, const uint32_t* counts,
                                  uint32_t uniform, kh_set** out) {
    if (!c || !out || (n && !keys_mixed)) return kh_fail(KH_E_ARG, "kh_set_wrap_device: bad argument");
    KHCHK(check_k(k));
    if (!n) { *out = make_set(k, 0, nullptr, 0, nullptr, 0, uniform ? uniform : 1); return KH_OK; }
    auto borrow = [&](const void* p, size_t bytes) {
        DevBuf* b = new DevBuf;
        b->p = const_cast<void*>(p);
        b->bytes = bytes;
        b->refs = 1;
        b->ctx = nullptr;   // not owned: never returned to the pool
        return b;
    };
    const int W = k <= 32 ? 1 : 2;
    DevBuf* kbuf = borrow(keys_mixed, 8 * (size_t)W * n);
    DevBuf* cbuf = counts ? borrow(counts, 4 * n) : nullptr;
    *out = make_set(k, n, kbuf, 0, cbuf, 0, uniform ? uniform : 1);
    return KH_OK;
}

extern "C" int kh_set_partition_bounds(kh_ctx* c, const kh_set* s, uint32_t nparts, uint64_t* bounds) {
    if (!c || !s || !bounds || !nparts) return kh_fail(KH_E_ARG, "kh_set_partition_bounds: bad argument");
    HIPCHK(hipSetDevice(c->dev));
    if (!s->n) { for (u64 i = 0; i <= nparts; ++i) bounds[i] = 0; return KH_OK; }   // u64: nparts may be 2^32 - 1
    KhSetView v{s->keys_ptr(), nullptr, s->n, 1, 0};
    Tmp d_view, d_bounds;
    TMP_ALLOC(d_view, c, sizeof v);
    TMP_ALLOC(d_bounds, c, 8 * ((u64)nparts + 1));
    HIPCHK(hipMemcpyAsync(d_view.b->p, &v, sizeof v, hipMemcpyHostToDevice, c->st));
    kh_launch_range_bounds(s->W, d_view.as<KhSetView>(), 1, nparts, s->k, d_bounds.as<u64>(), nullptr, 0, c->st);
    HIPCHK(hipMemcpyAsync(bounds, d_bounds.b->p, 8 * ((u64)nparts + 1), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return KH_OK;
}

extern "C" int kh_sets_partition_bounds(kh_ctx* c, const kh_set* const* sets, int nsets, uint32_t nparts,
                                        uint64_t* bounds) {
    if (!c || !sets || !bounds || !nparts || nsets <= 0) return kh_fail(KH_E_ARG, "kh_sets_partition_bounds: bad argument");
    for (int i = 0; i < nsets; ++i)
        if (!sets[i]) return kh_fail(KH_E_ARG, "kh_sets_partition_bounds: set %d is NULL", i);
    HIPCHK(hipSetDevice(c->dev));
    const int k = sets[0]->k, W = sets[0]->W;
    std::vector<KhSetView> v(nsets);
    for (int i = 0; i < nsets; ++i) {
        if (sets[i]->k != k) return kh_fail(KH_E_KMISMATCH, "sets built with different k");
        v[i] = KhSetView{sets[i]->n ? sets[i]->keys_ptr() : nullptr, nullptr, sets[i]->n, 1, 0};
    }
    Tmp d_view, d_bounds;
    const u64 nb = ((u64)nparts + 1) * nsets;
    TMP_ALLOC(d_view, c, sizeof(KhSetView) * nsets);
    TMP_ALLOC(d_bounds, c, 8 * nb);
    HIPCHK(hipMemcpyAsync(d_view.b->p, v.data(), sizeof(KhSetView) * nsets, hipMemcpyHostToDevice, c->st));
    kh_launch_range_bounds(W, d_view.as<KhSetView>(), nsets, nparts, k, d_bounds.as<u64>(), nullptr, 0, c->st);
    HIPCHK(hipMemcpyAsync(bounds, d_bounds.b->p, 8 * nb, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return KH_OK;
}

// ------------------------------------------------------------------------------ fused exp 1
// A group whose genomes do not fit the wave budget together ("HBM spill"):
// its genomes are built in sub-waves, each summed into a running union that carries counters
// (no saturation until the end), so the memory in flight is one sub-wave + the union.  The
// final pass applies `cs` and takes the histogram.  Same result as the one-wave path.
struct SetBag {   // sets that are freed on every way out
    std::vector<kh_set*> v;
    ~SetBag() { clear(); }
    void clear() {
        for (kh_set* s : v) kh_set_free(s);
        v.clear();
    }
    kh_set** slot() { v.push_back(nullptr); return &v.back(); }   // (valid until the next slot())
};
static int group_union_incremental(kh_ctx* c, const std::vector<int>& members, const uint8_t* const* seqs,
                                   const uint64_t* lens, int on_device, int k, u32 cs, u64 budget,
                                   uint64_t* hist, u32 hist_len, uint64_t* distinct_per_seq,
                                   kh_set** out_union) {
    kh_set* running = nullptr;
    SetBag wsets;
    size_t i0 = 0;
    while (i0 < members.size()) {
        size_t i1 = i0;
        u64 acc = 0;
        while (i1 < members.size() && (i1 == i0 || acc + lens[members[i1]] <= budget) &&
               i1 - i0 < (size_t)KH_MAX_INPUT_SETS - 1)
            acc += lens[members[i1++]];
        std::vector<const uint8_t*> wseqs(i1 - i0);
        std::vector<uint64_t> wlens(i1 - i0);
        wsets.v.assign(i1 - i0, nullptr);
        for (size_t j = i0; j < i1; ++j) { wseqs[j - i0] = seqs[members[j]]; wlens[j - i0] = lens[members[j]]; }
        int r = kh_build_batch(c, (int)(i1 - i0), wseqs.data(), wlens.data(), on_device, k, 1, KH_NO_MAX,
                               KH_KMC_DEFAULT_CS, 0, wsets.v.data());
        if (r != KH_OK) { kh_set_free(running); return r; }
        std::vector<const kh_set*> in;
        if (running) in.push_back(running);
        for (size_t j = i0; j < i1; ++j) {
            if (distinct_per_seq) distinct_per_seq[members[j]] = wsets.v[j - i0]->n;
            in.push_back(wsets.v[j - i0]);
        }
        kh_set* next = nullptr;
        r = run_setop(c, in, KH_OP_UNION, KH_OC_SUM, 0x7fffffffu, &next, nullptr, 0);
        if (r != KH_OK) { kh_set_free(running); return r; }
        wsets.clear();
        kh_set_free(running);
        running = next;
        i0 = i1;
    }
    std::vector<const kh_set*> in{running};
    const int r = run_setop(c, in, KH_OP_UNION, KH_OC_SUM, cs, out_union, hist, hist_len);
    kh_set_free(running);
    return r;
}

struct Exp1In {   // the arguments of kh_exp1_run that every form reads
    int nseq; const uint8_t* const* seqs; const uint64_t* lens; int on_device;
    const int* group_of; int ngroups, k; u32 cs, hist_len;
};
// The operands of a tagged union (exp1_skm, exp1_fused) in group-major order: the genomes of a group are consecutive
// bits of the mask.  Bins: per group one per count of its operands, then one per count of groups (across).  by_group:
// the operands are the GROUPS (every record carries its genome's group number): only the across-group histogram comes
// out — the second pass of a run over more than 64 genomes, whose batches have answered the within-group questions.
struct TagLayout {
    int nseq = 0, ngroups = 0;
    bool by_group = false;
    std::vector<int> gsize, gstart, perm;   // perm[i]: the caller's sequence that is operand i
    std::vector<u32> bin0;                  // first bin of a group
    u32 abase = 0, nbins = 0;               // first across-group bin, bins in all
    u32 fan = 1;                            // genomes of the largest group
    // [64] ginfo words; by_group: [nseq] the tag (group) of every operand
    void words(u32* h_ginfo, u8* h_tags, const int* group_of) const {
        memset(h_ginfo, 0, 256);
        if (by_group) {
            for (int g = 0; g < ngroups; ++g) h_ginfo[g] = (u32)g | (1u << 8) | (bin0[g] << 16);
            for (int i = 0; i < nseq; ++i) h_tags[i] = (u8)group_of[perm[i]];
        } else {
            for (int g = 0; g < ngroups; ++g)
                for (int j = 0; j < gsize[g]; ++j)
                    h_ginfo[gstart[g] + j] = (u32)gstart[g] | ((u32)gsize[g] << 8) | (bin0[g] << 16);
        }
    }
    void add_bins(std::vector<u64>& bins, const u64* h_hist, u32 reps) const {   // the kernels' per-workgroup copies
        for (u32 r = 0; r < reps; ++r)
            for (u32 b = 0; b < nbins; ++b) bins[b] += h_hist[(size_t)r * nbins + b];
    }
    void fold(kh_ctx* c, const std::vector<u64>& bins, uint64_t* within_hist, uint64_t* across_hist, u32 hist_len) const {
        if (within_hist && !by_group) {
            memset(within_hist, 0, 8 * (size_t)ngroups * hist_len);
            for (int g = 0; g < ngroups; ++g)
                for (int cnt = 1; cnt <= gsize[g]; ++cnt)
                    within_hist[(size_t)g * hist_len + std::min<u32>((u32)cnt, hist_len - 1)] += bins[bin0[g] + cnt];
        }
        u64 across_n = 0;
        for (int cnt = 1; cnt <= ngroups; ++cnt) across_n += bins[abase + cnt];
        c->stat.setop_out += across_n;
        if (across_hist) {
            memset(across_hist, 0, 8 * (size_t)hist_len);
            for (int cnt = 1; cnt <= ngroups; ++cnt)
                across_hist[std::min<u32>((u32)cnt, hist_len - 1)] += bins[abase + cnt];
        }
    }
};
static int tag_layout(TagLayout* L, int nseq, const int* group_of, int ngroups, bool by_group) {
    L->nseq = nseq;
    L->ngroups = ngroups;
    L->by_group = by_group;
    L->gsize.assign(ngroups, 0);
    L->gstart.assign(ngroups + 1, 0);
    L->perm.resize(nseq);
    L->bin0.resize(ngroups);
    for (int i = 0; i < nseq; ++i) L->gsize[group_of[i]]++;
    for (int g = 0; g < ngroups; ++g) {
        if (!L->gsize[g]) return kh_fail(KH_E_ARG, "group %d has no sequences", g);
        L->gstart[g + 1] = L->gstart[g] + L->gsize[g];
        L->bin0[g] = L->nbins;
        L->nbins += (by_group ? 1u : (u32)L->gsize[g]) + 1;   // by_group: every operand is a group of its own
        L->fan = std::max<u32>(L->fan, (u32)L->gsize[g]);
    }
    L->abase = L->nbins;
    L->nbins += (u32)ngroups + 1;
    std::vector<int> at(L->gstart.begin(), L->gstart.end() - 1);
    for (int i = 0; i < nseq; ++i) L->perm[at[group_of[i]]++] = i;
    return KH_OK;
}
static u64 kmer_positions(int n, const uint64_t* lens, int k, u64* bases = nullptr) {
    u64 pos = 0, b = 0;
    for (int i = 0; i < n; ++i) {
        pos += lens[i] >= (u64)k ? lens[i] - k + 1 : 0;
        b += lens[i];
    }
    if (bases) *bases = b;
    return pos;
}
// The super-k-mer form of the fused path (kh_skm.hip): bases -> 16-byte records of consecutive k-mers that
// share their minimizer slot -> two counting-sort levels (coarse bucket, slot) -> one LDS hash set per
// slot.  Takes what the key-array form below takes when k is in [KH_SKM_MIN_K, KH_SKM_MAX_K], nothing is
// emitted and the batch fits one slot grid; *done == false: not applicable, or a region overflowed
// (low-complexity input, far more records than estimated) — the caller goes on to the key-array form.
// Minimizer length of the one-word super-k-mer form.  A longer window (shorter minimizer) makes longer runs: fewer,
// longer records for all three kernels — as long as the 4^m minimizers still spread over the slots (m = 11 overfills
// too many).  Measured on the headline shape (ms per step, m = 15 / 13 / 12): k = 21 3.40 / 2.95 / 2.87, k = 24
// 2.84 / 2.60 / 2.57, k = 27 2.53 / 2.47 / 2.51; from k = 28 the record's 24 .. 27 k-mers are the limit, not the window
// (k = 30 .. 32: no difference): m = 16 where that makes the window a power of two, else 15.
static int skm_minimizer_len(int k) {
    if (k <= 24) return k >= 17 ? 12 : 11;   // k = 17 .. 24: 12 (k = 17: windows of 6, 3.75 ms against 4.6 with 11 bases and 4.4 with key
                                             // arrays); the kernels alone at k = 15, 16: 11
    if (k <= 27) return 13;
    const int m15w = k - 15 + 1;                                   // m-mers per k-mer with m = 15
    return (m15w > 1 && ((m15w - 1) & (m15w - 2)) == 0) ? 16 : 15;
}
static bool skm_form_k(int k) {
    // k = 17 .. 19 on the headline shape: 3.75 / 3.6 / 3.3 ms against 4.4 with key arrays; k = 16 and 15 (windows of 5
    // or 6 over 11 bases: too many overfull slots; over 12: twice the coarse buckets) 5.2 / 6.7 ms: below 17 the key
    // arrays stay (KHOICE_SKM_MIN_K: experiments and tests, the kernels take k >= 15)
    int min_k = KH_SKM_MIN_K;
    if (const char* e = getenv("KHOICE_SKM_MIN_K")) min_k = std::max(15, atoi(e));
    if (k < min_k || k > KH_SKM2_MAX_K || getenv("KHOICE_NO_SKM")) return false;
    return k <= KH_SKM_MAX_K || !getenv("KHOICE_NO_SKM2");   // two-word keys: 32-byte records, kh_skm2.hip
}
// records per k-mer: a run of k-mers with one minimizer is (w + 1) / 2 long on average; cuts at the waves' 2048
// positions, at boundaries a run may not cross (a second thread boundary, nmax) and at invalid bases add
// a little (measured: 0.120 records per k-mer at w = 16, 0.27 at w = 7)
static double skm_per_kmer(u32 w) { return 2.0 / (double)(w + 1) + 1.0 / 48.0; }
// k-mer instances that land in a slot together (the copies of a locus in the `fan` genomes of a group: skm_plan)
static double skm_clump(u32 w, u32 fan) { return 0.5 * (double)(w + 1) * (double)fan; }
// a slot's records vary like its instances: sigma / mean = sqrt(clump / mean) (12 % at k = 31 with groups of five,
// 36 % with ten genomes per group and two-word keys): five sigma, at least 1.7
static double skm_region_slack(double clump, double mean) { return std::max(1.7, 1.0 + 5.0 * std::sqrt(clump / mean)); }
// records of one part of the exchange form: the piece's records over nparts, 30 % to spare
static u64 skm_part_cap(u64 positions, double per_kmer, int nparts) {
    return ((u64)((double)positions * per_kmer * 1.3 / nparts) + 8192 + 63) & ~63ull;
}
struct SkmGeometry {
    const KhSkmWidth* wd = nullptr; // the key width's constants and launchers (kh_skm_width)
    bool two = false;               // two-word keys
    int m = 0;                      // minimizer length
    u32 w = 0, nmax = 0;            // m-mers per k-mer, k-mers per record at most
    u64 positions = 0;              // k-mer positions of the input
    u32 nslots = 0, S = 0, nb1 = 0; // slots, slots per coarse bucket, coarse buckets
    u32 cap1 = 0, cap2 = 0;         // records a coarse bucket's / a slot's region holds
    u32 ugrid = 0;                  // workgroups of the persistent union
};
// The slot geometry for `positions` k-mer positions whose largest group has `fan` genomes; force_slots: the number of
// slots all ranks agreed on (slots are a global function of the minimizer).  false: the form does not apply.
// table: the instances "mean + 2.5 sigma" aims at; 0: the table of the union of the key width.
static bool skm_plan(int k, u64 positions, u32 fan, u32 force_slots, int cus, SkmGeometry* out, u32 table = 0) {
    if (!skm_form_k(k)) return false;
    SkmGeometry g;
    g.two = k > KH_SKM_MAX_K;
    const KhSkmWidth& wd = kh_skm_width(g.two);
    g.wd = &wd;
    if (!g.two) {
        g.m = skm_minimizer_len(k);
        if (const char* e = getenv("KHOICE_SKM_M")) g.m = std::min(16, std::max(2, atoi(e)));   // experiments
        if (g.m >= k) return false;
        g.w = (u32)(k - g.m + 1);
        g.nmax = (u32)std::min(31, 55 - k);
        if (!wd.supports_w(g.w)) return false;
    } else {   // the scatter exists for every third window width: one of m = 16, 15, 14 fits
        g.m = 16;
        while (g.m >= 14 && !wd.supports_w((u32)(k - g.m + 1))) --g.m;
        if (g.m < 14) return false;
        g.w = (u32)(k - g.m + 1);
        g.nmax = (u32)std::min(63, 118 - k);
    }
    if (!positions) return false;
    g.positions = positions;
    // k-mer instances per slot: the hash set takes T = 4096 (2048 for two-word keys) per round.  The genomes of a
    // group put their copies of a locus in the same slot, a minimizer run at a time: clumps of c = (w + 1) / 2 x
    // (largest group) instances, so sigma = sqrt(mean x c); mean + 2.5 sigma = T  (measured: 2500 / 2900 / 3200 /
    // 3500 / 3800 at k = 31 with groups of five: union 1.96 / 1.81 / 1.75 / 1.80 / 1.94 ms; the rule gives 3180)
    const double clump = skm_clump(g.w, fan);
    const double T = table ? (double)table : (double)wd.table;
    const double r = 0.5 * (-2.5 * std::sqrt(clump) + std::sqrt(6.25 * clump + 4.0 * T));
    u32 mean = (u32)std::max(256.0, r * r);
    if (const char* e = getenv("KHOICE_SKM_MEAN")) mean = std::max<u32>(64, (u32)strtoul(e, nullptr, 10));
    const double per_kmer = skm_per_kmer(g.w);
    double slack1 = 1.25, slack2 = 1.7;
    const u32 max_cap2 = wd.max_cap2;
    for (int it = 0; it < 8; ++it) {   // short windows (k = 20 .. 22: 3.5 k-mers per record): fewer instances per slot so that its records fit
        slack2 = skm_region_slack(clump, (double)mean);
        const double c2 = (double)mean * per_kmer * slack2 + 96 + 16;
        if (c2 <= (double)max_cap2 || mean <= 256) break;
        mean = std::max<u32>(256, (u32)((double)mean * (double)max_cap2 / c2 * 0.98));
    }
    u64 nslots64 = force_slots ? force_slots : std::max<u64>(1, (positions + mean - 1) / mean);
    bool fuller = false;   // the slots hold more than `mean` (callers with a `table` only)
    // One-word keys a little above 256 x 512 slots (short windows on the headline shape: k = 20): 512 coarse buckets
    // double the scatter's cursors and LDS (k = 20: scatter 2.3 ms against 1.0 at k = 21).  Since a slot's region may
    // overflow (side list, k_skm_big) its slack can be cut instead: stay at 256 x 512 slots with slack down to 1.4.
    // Two-word keys a little above 512 x 1024 slots (configs[2] at k = 41, the pass by group over 500 M positions):
    // the same cut, up to what the union's table takes in one go on average.
    const u64 lim = (u64)wd.max_coarse * wd.max_fine;
    if (!force_slots && nslots64 > lim) {
        const double per_slot = (double)positions * per_kmer / (double)lim;
        const double s2 = ((double)max_cap2 - 112.0) / per_slot;
        if (s2 >= 1.4 && (!g.two || (double)positions / (double)lim <= 0.75 * (double)wd.table)) {
            nslots64 = lim;
            slack2 = std::min(slack2, s2);
        }
    }
    // coarse buckets: 256 keep the scatter's runs long; inputs past 256 x 512 slots (> 400 M k-mers) take 512
    const u32 max_coarse = nslots64 > lim ? kh_skm_width(true).max_coarse : wd.max_coarse;   // (one-word keys past their own limit: the two-word scatter's 512)
    if (nslots64 > (u64)max_coarse * wd.max_fine) {
        // more slots than the two levels number.  A caller whose kernel takes a slot in rounds (`table`: k_skm_cross)
        // gets all of them, fuller than the rule wants — as long as a region with its whole slack holds their records
        // (below; measured without that condition at k = 17 on 625 Mbp: regions cut to 1.4 x the mean, more records
        // spilled than the side list keeps, the call paid 15 ms for the attempt before the set form answered)
        if (!table || force_slots) return false;
        nslots64 = (u64)max_coarse * wd.max_fine;
        fuller = true;
    }
    g.nslots = (u32)nslots64;
    g.S = std::max<u32>(1, (g.nslots + max_coarse - 1) / max_coarse);
    g.nb1 = (g.nslots + g.S - 1) / g.S;
    const double recs = (double)positions * per_kmer;
    if (const char* e = getenv("KHOICE_SKM_SLACK")) slack1 = slack2 = std::max(0.01, atof(e));   // below 1: tests of the overflow fall-back
    const u64 cap1_64 = ((u64)(recs / g.nb1 * slack1) + 2048 + 63) & ~63ull;
    u64 cap2_64 = ((u64)(recs / g.nslots * slack2) + 96 + 15) & ~15ull;
    if (cap2_64 > max_cap2 && !force_slots && !fuller) {
        // Large groups: the copies of a locus (one record per genome of the group) arrive in a slot together, so the
        // five-sigma region is larger than the union takes.  The region is cut to what it takes and the slots with a
        // locus too many go the side-list way (k_skm_big); only when there are more of those than the side list
        // holds is the call given to the key arrays.  (Models of how many there will be — loci per slot Poisson, the
        // group's genomes as one clump — were off by 10 x in both directions on synthetic sets: it is tried.)
        if ((double)fan + recs / (double)g.nslots <= (double)max_cap2 - 112.0) cap2_64 = max_cap2 & ~15u;
    }
    if (cap2_64 > max_cap2 || cap1_64 > 0x7fffffffull) return false;
    g.cap1 = (u32)cap1_64;
    g.cap2 = (u32)cap2_64;
    // the union is persistent (as many workgroups as fit the chip, each with a histogram of its own)
    g.ugrid = std::min<u32>(g.nslots, wd.union_per_cu * (u32)std::max(1, cus));
    *out = g;
    return true;
}
// a launch under its profiling class, and the error it may have left
template <class F> static int timed_launch(kh_ctx* c, int cls, F launch) {
    c->prof_begin(cls);
    launch();
    c->prof_end();
    HIPCHK(hipGetLastError());
    return KH_OK;
}
// One run of a super-k-mer form, what exp1_skm, exp3_skm and skm_pack_impl do alike.  In this order: skm_prepare() (the
// geometry, the texts, scatter and regroup; !staged: the form does not apply); the form's own launch over the records
// by slot; settle() (exp1_skm, exp3_skm) or read_back() (skm_pack_impl); then h_ctl(), h_hist() and per_text().
// Workspace: [hist: reps x nbins u64][ctl: KH_SKM_CTL_WORDS u32][inst: nseq u64][dup: 64 u64] (zeroed, read back)
// [cur1: nb1 x KH_SKM_CUR1_STRIDE u32][cur2: nslots u32][claim: a 128-byte line of its own] (zeroed) [ginfo: 64 u32]
// [tags: nseq u8][segs][tiles] (fetched from the pinned staging).  No copy engine on the way: k_skm_ws_init zeroes and
// fetches in front of the scatter, k_skm_ws_down stores [hist .. dup] to the pinned staging behind the form's kernel.
struct SkmRun {
    kh_ctx* c;
    TagLayout L;
    SkmGeometry g;
    KhSkmJob job;
    struct Layout { size_t ctl, inst, dup, cur1, cur2, claim, ginfo, tags, segs, tiles, bytes; } off{};   // (hist at 0)
    TextStage texts;
    Tmp d_ws, d_reg1, d_reg2, d_spill;
    Pinned pin;
    u8* h_down = nullptr;           // pinned read-back of the workspace's [hist .. dup], laid out as on the device
    u32 ntiles = 0;
    u64 bases = 0;
    bool staged = false;            // false: the form does not apply (k, operands, geometry, memory)
    // what a slot's region cannot hold goes to a side list (d_spill: [spill_cap] records, [spill_cap] u32 slots, [big_cap]
    // u32 listed slots), the slot to a launch of its own
    static constexpr u32 spill_cap = 1u << 20, big_cap = 16384u;
    // Replicas of the histogram: a union workgroup adds its bins to replica blockIdx.x % reps once, at its end, so a few
    // spread those atomics enough (union time with 1 / 4 / 8 / 32 / one per workgroup: 1.226 / 1.224 / 1.225 / 1.226 /
    // 1.223 ms), and what is zeroed, read back and summed per call shrinks from 290 KB to 5 KB on the headline shape
    static constexpr u32 hist_reps = 8u;
#ifdef KH_STAMPS
    Tmp d_stamps;
#endif
    explicit SkmRun(kh_ctx* ctx) : c(ctx), pin{ctx} {}

    void layout(size_t hist_words, int nseq) {
        off.ctl = 8 * hist_words;
        off.inst = off.ctl + 4 * (size_t)KH_SKM_CTL_WORDS;
        off.dup = off.inst + 8 * (size_t)nseq;
        off.cur1 = off.dup + 8 * 64;
        off.cur2 = off.cur1 + 4 * (size_t)KH_SKM_CUR1_STRIDE * g.nb1;
        off.claim = (off.cur2 + 4 * (size_t)g.nslots + 127) & ~(size_t)127;
        off.ginfo = off.claim + 128;
        off.tags = off.ginfo + 256;
        off.segs = off.tags + (((size_t)nseq + 15) & ~(size_t)15);
        off.tiles = off.segs + sizeof(KhSeg) * nseq;
        off.bytes = (off.tiles + sizeof(KhTile) * (size_t)std::max<u32>(1, ntiles) + 15) & ~(size_t)15;   // (fetched in 16-byte words)
    }
    template <class T> T* dev(size_t o) const { return reinterpret_cast<T*>(d_ws.as<u8>() + o); }
    // [from, dup's end) of the workspace into h_down, and the wait for it
    int read_back(size_t from) {
        kh_launch_skm_ws_down(h_down + from, d_ws.as<u8>() + from, off.cur1 - from, c->st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(c->st));
        return KH_OK;
    }
    const u64* h_hist() const { return reinterpret_cast<const u64*>(h_down); }             // [reps][nbins]
    const u32* h_ctl() const { return reinterpret_cast<const u32*>(h_down + off.ctl); }    // [KH_SKM_CTL_WORDS]
    const u64* h_inst() const { return reinterpret_cast<const u64*>(h_down + off.inst); }  // [nseq]
    const u64* h_dup() const { return reinterpret_cast<const u64*>(h_down + off.dup); }    // [64]
    bool failed() const { return (h_ctl()[KH_SKM_CTL_ERR] & (KH_ERR_CAPACITY | KH_ERR_ORDER)) != 0; }
    // After the form's first launch: [from, dup's end) read back; overfull slots (skewed input: a minimizer shared by far
    // more k-mers than a hash predicts) were listed and left out — listed(n) launches the kernel that takes the n of them
    // (only these slots are done twice, not the call), and the read-back again.  *declines (retries counted): more
    // spilled records or listed slots than are kept, or a region, a slot or a table overflowed; another form answers.
    template <class F> int settle(size_t from, F listed, bool* declines) {
        *declines = true;
        KHCHK(read_back(from));
        const u32* hc = h_ctl();
        if (hc[KH_SKM_CTL_LISTED] && !failed()) {
            if (hc[KH_SKM_CTL_SPILLED] > spill_cap || hc[KH_SKM_CTL_LISTED] > big_cap) { c->stat.retries++; return KH_OK; }
            KHCHK(listed(hc[KH_SKM_CTL_LISTED]));
            KHCHK(read_back(from));
        }
        if (failed()) { c->stat.retries++; return KH_OK; }
        *declines = false;
        return KH_OK;
    }
    // f(t, instances, distinct) for every operand: the caller's text t, its valid k-mer instances, and (after the union
    // or the cross kernel) its distinct k-mers = instances minus those whose (k-mer, operand) pair was seen before
    template <class F> void per_text(F f) const {
        for (int i = 0; i < L.nseq; ++i) f(L.perm[i], h_inst()[i], h_inst()[i] - h_dup()[i]);
    }
};
// (a) + (b): the geometry, then the input staged, scattered and regrouped by slot
static int skm_prepare(kh_ctx* c, int nseq, const uint8_t* const* seqs, const uint64_t* lens, int on_device,
                       const int* group_of, int ngroups, int k, bool by_group, u32 force_slots, u32 fan_hint, SkmRun* s,
                       u32 table = 0 /* skm_plan's: 0 for the unions */) {
    TagLayout* L = &s->L;
    if (!skm_form_k(k)) return KH_OK;
    if ((!by_group && nseq > KH_TAG_MAX_OPS) || ngroups > KH_TAG_MAX_OPS) return KH_OK;
    KHCHK(tag_layout(L, nseq, group_of, ngroups, by_group));
    if (L->nbins > (u32)KH_TAG_MAX_BINS) return KH_OK;
    const u64 positions = kmer_positions(nseq, lens, k, &s->bases);
    // (fan_hint: genomes whose copies of a locus arrive together although they are tags of ONE group)
    if (!skm_plan(k, positions, std::max(L->fan, fan_hint), force_slots, c->cus, &s->g, table)) return KH_OK;
    const SkmGeometry& g = s->g;
    const KhSkmWidth& wd = *g.wd;
    const size_t rec_bytes = wd.rec_bytes;
    const size_t reg1_bytes = rec_bytes * (size_t)g.nb1 * g.cap1, reg2_bytes = rec_bytes * (size_t)g.nslots * g.cap2;
    HIPCHK(hipSetDevice(c->dev));
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
            reg1_bytes + reg2_bytes + s->bases + (64u << 20) > free_b + c->pool.cached_bytes)
            return KH_OK;   // the key-range waves of the key-array form handle what does not fit
    }
    hipStream_t st = c->st;

    // ---- segments and tiles (operands in group-major order: the genomes of a group are consecutive mask bits)
    u32 tile_pos = KH_TILE;
    {
        const u64 want_tiles = 8ull * (u64)std::max(1, c->cus);
        while (tile_pos > (u32)KH_SUBTILE && (positions + tile_pos - 1) / tile_pos < want_tiles) tile_pos >>= 1;
    }
    std::vector<KhSeg> segs(nseq);
    std::vector<KhTile> tiles;
    for (int i = 0; i < nseq; ++i) {
        KhSeg& sg = segs[i];
        memset(&sg, 0, sizeof sg);
        const u64 len = lens[L->perm[i]];
        sg.len = len;
        sg.npos = len >= (u64)k ? len - k + 1 : 0;
        sg.ntiles = (u32)((sg.npos + tile_pos - 1) / tile_pos);
        sg.tile_base = (u32)tiles.size();
        for (u32 t = 0; t < sg.ntiles; ++t) tiles.push_back(KhTile{(u32)i, t});
    }
    const u32 ntiles = s->ntiles = (u32)tiles.size();
    const u32 reps = std::min(g.ugrid, SkmRun::hist_reps);
    s->layout((size_t)reps * L->nbins, nseq);
    const SkmRun::Layout& off = s->off;
    const u32 spill_cap = SkmRun::spill_cap;
    TMP_ALLOC(s->d_ws, c, off.bytes);
    TMP_ALLOC(s->d_reg1, c, reg1_bytes);
    TMP_ALLOC(s->d_reg2, c, reg2_bytes);
    TMP_ALLOC(s->d_spill, c, (size_t)spill_cap * (rec_bytes + 4) + (size_t)SkmRun::big_cap * 4);
    // pinned staging: [ginfo][tags][segs][tiles] up, [hist .. dup] down
    const size_t up_bytes = off.bytes - off.ginfo;   // the upload, laid out as on the device
    PIN_ALLOC(s->pin, up_bytes + off.cur1 + 64);
    u8* h_up = static_cast<u8*>(s->pin.p);
    s->h_down = h_up + ((up_bytes + 63) & ~(size_t)63);
    c->prof_begin(KC_COPY_IN);
    KHCHK(s->texts.copy_in(c, nseq, seqs, lens, on_device, L->perm.data()));
    for (int i = 0; i < nseq; ++i) segs[i].seq = s->texts.dev[i];
    memcpy(h_up + (off.segs - off.ginfo), segs.data(), sizeof(KhSeg) * nseq);
    if (ntiles) memcpy(h_up + (off.tiles - off.ginfo), tiles.data(), sizeof(KhTile) * (size_t)ntiles);
    L->words(reinterpret_cast<u32*>(h_up), h_up + (off.tags - off.ginfo), group_of);
    kh_launch_skm_ws_init(s->d_ws.b->p, off.ginfo, h_up, up_bytes, st);
    HIPCHK(hipGetLastError());
    c->prof_end();

    KhSkmJob& job = s->job;
    job.seg_tag = by_group ? s->dev<const u8>(off.tags) : nullptr;
    job.segs = s->dev<const KhSeg>(off.segs);
    job.tiles = s->dev<const KhTile>(off.tiles);
    job.reg1 = s->d_reg1.as<uint4>();
    job.reg2 = s->d_reg2.as<uint4>();
    job.cur1 = s->dev<u32>(off.cur1);
    job.cur2 = s->dev<u32>(off.cur2);
    job.inst = s->dev<unsigned long long>(off.inst);
    job.dup = s->dev<unsigned long long>(off.dup);
    job.ginfo = s->dev<const u32>(off.ginfo);
    job.hist = s->dev<unsigned long long>(0);
    job.ctl = s->dev<u32>(off.ctl);
    job.claim = s->dev<u32>(off.claim);
    job.tile_pos = tile_pos;
    job.k = k; job.m = g.m; job.w = g.w; job.nmax = g.nmax;
    job.nslots = g.nslots; job.S = g.S; job.nb1 = g.nb1; job.cap1 = g.cap1; job.cap2 = g.cap2;
    job.nbins = L->nbins; job.abase = L->abase; job.reps = reps; job.nops = by_group ? (u32)ngroups : (u32)nseq;
    job.spill_rec = s->d_spill.as<uint4>();
    job.spill_slot = reinterpret_cast<u32*>(s->d_spill.as<u8>() + (size_t)spill_cap * rec_bytes);
    job.big_list = reinterpret_cast<u32*>(s->d_spill.as<u8>() + (size_t)spill_cap * (rec_bytes + 4));
    job.spill_cap = spill_cap;
    job.big_cap = SkmRun::big_cap;
#ifdef KH_STAMPS
    const u64 nst = std::max<u64>(ntiles, g.nslots);
    TMP_ALLOC(s->d_stamps, c, 128 * nst);
    HIPCHK(hipMemsetAsync(s->d_stamps.b->p, 0, 128 * nst, st));
    kh_debug_set_stamps_skm(s->d_stamps.as<u64>());
#endif
    c->prof_begin(KC_SKM_SCATTER);
    wd.scatter(job, ntiles, st);
    c->prof_end();
#if defined(KH_STAMPS) && defined(KH_STAMPS_WG)
    dump_wg_ends(c, s->d_stamps.b, ntiles, true);
    HIPCHK(hipMemsetAsync(s->d_stamps.b->p, 0, 128 * nst, st));
    kh_debug_set_stamps_skm(nullptr);
#elif defined(KH_STAMPS)
    report_stamps(c, "skm_scatter (second sub-tile: codes / hashes / minima / slots+count / - / append / barrier / -)", s->d_stamps.b, ntiles);
    HIPCHK(hipMemsetAsync(s->d_stamps.b->p, 0, 128 * nst, st));
    kh_debug_set_stamps_skm(nullptr);
#endif
    c->prof_begin(KC_SKM_REGROUP);
    wd.regroup(job, st);
    c->prof_end();
#ifdef KH_STAMPS
    kh_debug_set_stamps_skm(s->d_stamps.as<u64>());
#ifdef KH_STAMPS_WG
    kh_debug_set_stamps_skm2(s->d_stamps.as<u64>());
#endif
#endif
    s->staged = true;
    return KH_OK;
}
// (a) + (b) + (c): the union over the staged records (and k_skm_big for the slots it left out), then the read-out
static int exp1_skm(kh_ctx* c, const Exp1In& in, uint64_t* within_hist, uint64_t* across_hist, uint64_t* distinct_per_seq,
                    bool* done, bool by_group = false) {
    *done = false;
    SkmRun s(c);
    KHCHK(skm_prepare(c, in.nseq, in.seqs, in.lens, in.on_device, in.group_of, in.ngroups, in.k, by_group, 0, 0, &s));
    if (!s.staged) return KH_OK;
    const TagLayout& L = s.L;
    const SkmGeometry& g = s.g;
    const KhSkmJob& job = s.job;
    hipStream_t st = c->st;
    KHCHK(timed_launch(c, KC_SKM_UNION, [&] { g.wd->unite(job, in.cs, g.ugrid, st); }));
#if defined(KH_STAMPS) && defined(KH_STAMPS_WG)
    dump_wg_ends(c, s.d_stamps.b, g.ugrid);
    kh_debug_set_stamps_skm(nullptr);
    kh_debug_set_stamps_skm2(nullptr);
#elif defined(KH_STAMPS)
    report_stamps(c, "skm_union (scan barrier / owner / expand / insert / barrier / read-out / barrier / flush)", s.d_stamps.b, g.nslots);
    kh_debug_set_stamps_skm(nullptr);
#endif
    if (getenv("KHOICE_SKM_DEBUG")) {   // diagnostics: how full the regions are
        std::vector<u32> h1(g.nb1), h2(g.nslots);
        HIPCHK(hipMemcpy2DAsync(h1.data(), 4, job.cur1, 4 * (size_t)KH_SKM_CUR1_STRIDE, 4, g.nb1, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h2.data(), job.cur2, 4 * (size_t)g.nslots, hipMemcpyDeviceToHost, st));
        u32 hc[KH_SKM_CTL_WORDS];
        HIPCHK(hipMemcpyAsync(hc, job.ctl, sizeof hc, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        u64 t1 = 0, t2 = 0;
        u32 m1 = 0, m2 = 0;
        for (u32 v : h1) { t1 += v; m1 = std::max(m1, v); }
        for (u32 v : h2) { t2 += v; m2 = std::max(m2, v); }
        fprintf(stderr, "[skm] k=%d m=%d w=%u nmax=%u positions=%llu records=%llu (%.2f k-mers each) nb1=%u S=%u nslots=%u | "
                        "coarse: mean %.0f max %u cap %u | slot: mean %.1f max %u cap %u | tiles %u x %u | expanded: %u k-mers | errors %u spilled %u overfull slots %u multi-subset slots %u\n",
                in.k, g.m, g.w, g.nmax, (unsigned long long)g.positions, (unsigned long long)t1, (double)g.positions / std::max<u64>(1, t1),
                g.nb1, g.S, g.nslots, (double)t1 / g.nb1, m1, g.cap1, (double)t2 / g.nslots, m2, g.cap2, s.ntiles, job.tile_pos,
                hc[KH_SKM_CTL_EXPANDED], hc[KH_SKM_CTL_ERR], hc[KH_SKM_CTL_SPILLED], hc[KH_SKM_CTL_LISTED], g.two ? 0u : hc[KH_SKM_CTL_MULTI]);
    }
    bool declines = false;
    KHCHK(s.settle(0, [&](u32 nbig) {
        c->stat.big_slots += nbig;
        return timed_launch(c, KC_SKM_BIG, [&] { g.wd->big(job, in.cs, nbig, st); });
    }, &declines));
    if (declines) return KH_OK;   // the key-array form takes over
    c->stat.skm_records += s.h_ctl()[KH_SKM_CTL_RECORDS];
    if (!L.by_group) {
        c->stat.bases += s.bases;
        c->stat.builds += L.nseq;
        u64 isum = 0, dsum = 0;
        s.per_text([&](int t, u64 inst, u64 d) {
            isum += inst;
            dsum += d;
            if (distinct_per_seq) distinct_per_seq[t] = d;
        });
        c->stat.kmers += isum;
        c->stat.distinct += dsum;
        c->stat.setop_in += dsum;
    }
    c->stat.setops++;
    std::vector<u64> bins(L.nbins, 0);
    L.add_bins(bins, s.h_hist(), job.reps);
    L.fold(c, bins, within_hist, across_hist, in.hist_len);
    *done = true;
    return KH_OK;
}
// ------------------------------------------------------------------------------ exchange form of steps 7-8
// Multi-GPU (khoice_amd/dist.py): every rank turns its genomes into records tagged with the LOCAL group number,
// merges identical ones and packs them by the rank that owns their slot (kh_skm_pack); the packed arrays travel
// (all-to-all); the owner runs ONE phased union over the pieces it received (kh_skm_phased_histogram) and the small
// histograms are all-reduced.  Slot geometry must be the same on all ranks: kh_skm_exchange_plan works it out from
// numbers the ranks have agreed on (the largest rank's k-mer positions, the largest group).
static bool skm_exchange_k(int k) { return k >= KH_SKM_MIN_K && k <= KH_SKM_MAX_K; }

// slots for `nparts` pieces of at most positions_max k-mer positions each; false: too many k-mers per piece
static bool skm_exchange_geometry(int k, uint64_t positions_max, int nparts, u32 fan, u64* nslots, double* per_kmer_out,
                                  double eff_parts = 0.0 /* pieces that share most k-mers count as fewer; 0: nparts */) {
    const int m = skm_minimizer_len(k);
    const u32 w = (u32)(k - m + 1);
    const double per_kmer = skm_per_kmer(w);
    // k-mer instances per slot and rank.  The owner's table (4096 entries) takes ~3000 instances per round: with
    // groups of related genomes about 0.55 of a rank's instances survive the merge of identical records, so
    // 2600 / (0.55 x nparts) per rank keeps the owner at one round (unrelated genomes: two).  A rank's slot must also
    // fit the pack kernel's 1024 records, and the two partition levels give 512 x 512 slots at most (beyond: the
    // slots grow and the owner takes more rounds).
    // The regions of a rank's slots are sized as exp1_skm sizes them (skm_region_slack): they must stay below the pack
    // kernel's 1024 records.
    const double clump = skm_clump(w, std::max<u32>(1, fan));
    auto region = [&](double mean) { return mean * per_kmer * skm_region_slack(clump, mean) + 128.0; };
    if (eff_parts <= 0.0) eff_parts = (double)nparts;
    double mean = std::min(2600.0 / (0.55 * eff_parts), (1024.0 - 128.0) / (1.7 * per_kmer));
    while (mean > 64.0 && region(mean) > 1008.0) mean *= 0.95;
    if (const char* e = getenv("KHOICE_SKM_EXCHANGE_MEAN")) mean = std::max(16.0, atof(e));   // tests: rounds on the owner
    u64 ns = std::max<u64>((u64)nparts, (u64)((double)std::max<u64>(1, positions_max) / mean) + 1);
    ns = std::min<u64>(ns, (u64)KH_SKM2_MAX_COARSE * KH_SKM_MAX_FINE);
    if (region((double)positions_max / (double)ns) > 1024.0) return false;
    *nslots = ns;
    *per_kmer_out = per_kmer;
    return true;
}
extern "C" int kh_skm_exchange_plan(kh_ctx* c, int k, uint64_t positions_max, uint32_t fan_max, int nparts, uint32_t* nslots,
                                    uint32_t* slots_per_part, uint64_t* part_cap) {
    if (!c || !nslots || !slots_per_part || !part_cap || nparts < 1) return kh_fail(KH_E_ARG, "kh_skm_exchange_plan: bad argument");
    if (!skm_exchange_k(k)) return kh_fail(KH_E_ARG, "the exchange form takes k = %d .. %d", KH_SKM_MIN_K, KH_SKM_MAX_K);
    u64 ns = 0;
    double per_kmer = 0;
    if (!skm_exchange_geometry(k, positions_max, nparts, fan_max, &ns, &per_kmer))
        return kh_fail(KH_E_CAPACITY, "too many k-mers per rank for the exchange form (%llu positions)", (unsigned long long)positions_max);
    *nslots = (u32)ns;
    *slots_per_part = (u32)((ns + nparts - 1) / nparts);
    *part_cap = skm_part_cap(positions_max, per_kmer, nparts);
    return KH_OK;
}

// The one-GPU use of kh_skm_pack (a group of more than 64 genomes in sub-batches, exp1_big_group_skm): the tags are
// genomes of ONE group, whose copies of a locus arrive together.
struct SkmPackLocal {
    std::vector<u64> inst;   // out: k-mer instances per sequence, in the caller's order
    u64 dup[32] = {};        // out: instances whose (k-mer, tag) pair was seen before
    Tmp spill;               // out: records that did not fit their slot's region: [SkmRun::spill_cap] records, then as many u32 slots
    u32 spill_n = 0;
    bool done = false;       // what does not fit: false instead of an error
};
// The records by slot, (a) + (b) with the slots all ranks agreed on, packed by the part that owns their slot
static int skm_pack_impl(kh_ctx* c, int nseq, const uint8_t* const* seqs, const uint64_t* lens, int on_device,
                         const int* tag_of, int k, uint32_t nslots, int nparts, uint64_t part_cap, void* rec_out,
                         uint32_t* mask_out, uint32_t* count_out, uint32_t* off_out, uint64_t* part_n, SkmPackLocal* loc) {
    if (loc) loc->done = false;
    if (!c || nseq < 0 || (nseq && (!seqs || !lens || !tag_of)) || nparts < 1 || !nslots || !rec_out || !mask_out || !count_out ||
        !off_out || !part_n)
        return kh_fail(KH_E_ARG, "kh_skm_pack: bad argument");
    if (!skm_exchange_k(k)) return kh_fail(KH_E_ARG, "the exchange form takes k = %d .. %d", KH_SKM_MIN_K, KH_SKM_MAX_K);
    int ntags = 0;
    for (int i = 0; i < nseq; ++i) {
        if (tag_of[i] < 0 || tag_of[i] >= 32) return kh_fail(KH_E_ARG, "kh_skm_pack: tag %d outside 0..31", tag_of[i]);
        ntags = std::max(ntags, tag_of[i] + 1);
    }
    HIPCHK(hipSetDevice(c->dev));
    hipStream_t st = c->st;
    {   // every tag needs a sequence for the geometry code (groups without genomes are refused there): tags are dense here
        std::vector<int> seen(ntags, 0);
        for (int i = 0; i < nseq; ++i) seen[tag_of[i]] = 1;
        for (int t = 0; t < ntags; ++t)
            if (!seen[t]) return kh_fail(KH_E_ARG, "kh_skm_pack: tag %d has no sequence", t);
    }
    const u32 spp = (nslots + (u32)nparts - 1) / (u32)nparts;
    if (!loc && !kmer_positions(nseq, lens, k)) {
        // a rank without k-mers (no sequences, or all shorter than k) still sends its parts: all empty
        HIPCHK(hipMemsetAsync(count_out, 0, 4 * (size_t)spp * nparts, st));
        HIPCHK(hipMemsetAsync(off_out, 0, 4 * (size_t)spp * nparts, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int p = 0; p < nparts; ++p) part_n[p] = 0;
        return KH_OK;
    }
    SkmRun s(c);
    KHCHK(skm_prepare(c, nseq, seqs, lens, on_device, tag_of, ntags, k, /*by_group=*/true, nslots, loc ? (u32)nseq : 0u, &s));
    u32 spilled = 0;
    if (s.staged) {
        HIPCHK(hipGetLastError());
        KHCHK(s.read_back(s.off.ctl));   // the control words and the instances per sequence
        const u32* h_ctl = s.h_ctl();
        spilled = h_ctl[KH_SKM_CTL_SPILLED];
        if (getenv("KHOICE_SKM_DEBUG"))
            fprintf(stderr, "[skm records] k=%d positions=%llu nb1=%u S=%u nslots=%u cap1 %u cap2 %u | records %u errors %u spilled %u\n", k,
                    (unsigned long long)s.g.positions, s.g.nb1, s.g.S, s.g.nslots, s.g.cap1, s.g.cap2, h_ctl[KH_SKM_CTL_RECORDS],
                    h_ctl[KH_SKM_CTL_ERR], spilled);
        // (records on the side list: handed out to a caller that asked for them, a failure otherwise)
        if (s.failed() || (spilled && (!loc || s.g.two || spilled > SkmRun::spill_cap))) {
            c->stat.retries++;
            s.staged = false;
        }
    }
    if (!s.staged) {
        if (loc) return KH_OK;
        return kh_fail(KH_E_CAPACITY, "kh_skm_pack: the records did not fit their regions (low-complexity input?)");
    }
    if (spilled) {
        loc->spill.b = s.d_spill.b; s.d_spill.b = nullptr;
        loc->spill_n = spilled;
    }
    c->stat.skm_records += s.h_ctl()[KH_SKM_CTL_RECORDS];
    if (loc) {
        loc->inst.assign(nseq, 0);
        s.per_text([&](int t, u64 inst, u64) { loc->inst[t] = inst; });
    }
    for (Tmp* t : {&s.texts.d_seq, &s.d_reg1, &s.d_spill}) { buf_unref(t->b); t->b = nullptr; }   // from here on: the records by slot
    Tmp d_ctl;
    u32 nsub = loc ? 64u : 1u;   // (the one-GPU use: 64 cursors into its one part, which does not travel)
    // The caller wants every part without gaps (it travels): packed through 64 cursors into a buffer of our own and
    // moved together afterwards — one cursor per part is a queue of returning atomics (78 K slots: 0.8 ms).
    const bool compact = nsub == 1 && spp >= 2048;
    if (compact) nsub = 64;
    // the pack's control block: [KH_SKM_XCTL_CURSORS u32][cursors: nparts x nsub u32][part_n: nparts u32][dup: 32 u64]
    const size_t off_cursors = 4 * (size_t)KH_SKM_XCTL_CURSORS, off_part_n = (off_cursors + 4 * (size_t)nparts * nsub + 7) & ~(size_t)7,
                 off_dup = off_part_n + ((4 * (size_t)nparts + 7) & ~(size_t)7), ctl_bytes = off_dup + 8 * 32;
    Tmp d_tmp;
    if (compact) TMP_ALLOC(d_tmp, c, (size_t)nparts * part_cap * 20);
    TMP_ALLOC(d_ctl, c, ctl_bytes);
    HIPCHK(hipMemsetAsync(d_ctl.b->p, 0, ctl_bytes, st));
    HIPCHK(hipMemsetAsync(count_out, 0, 4 * (size_t)spp * nparts, st));   // (slots past the last one: nothing)
    HIPCHK(hipMemsetAsync(off_out, 0, 4 * (size_t)spp * nparts, st));
    KhSkmPackJob job;
    job.reg2 = s.d_reg2.as<uint4>();
    job.cur2 = s.job.cur2;
    job.out_rec = compact ? d_tmp.as<uint4>() : static_cast<uint4*>(rec_out);
    job.out_mask = compact ? reinterpret_cast<u32*>(d_tmp.as<u8>() + 16 * (size_t)nparts * part_cap) : mask_out;
    job.part_cursor = d_ctl.as<u32>() + KH_SKM_XCTL_CURSORS;
    job.slot_count = count_out;
    job.slot_off = off_out;
    job.ctl = d_ctl.as<u32>();
    job.dup = loc ? reinterpret_cast<unsigned long long*>(d_ctl.as<u8>() + off_dup) : nullptr;
    job.part_cap = part_cap;
    job.cap2 = s.g.cap2;
    job.nslots = s.g.nslots;
    job.spp = spp;
    job.nsub = nsub;
    c->prof_begin(KC_SKM_PACK);
    kh_launch_skm_pack(job, st);
    if (compact) {
        KhSkmCompactJob cj;
        cj.tmp_rec = job.out_rec;
        cj.tmp_mask = job.out_mask;
        cj.out_rec = static_cast<uint4*>(rec_out);
        cj.out_mask = mask_out;
        cj.cursors = job.part_cursor;
        cj.slot_off = off_out;
        cj.part_n = reinterpret_cast<u32*>(d_ctl.as<u8>() + off_part_n);
        cj.part_cap = part_cap;
        cj.nslots = s.g.nslots;
        cj.spp = spp;
        cj.nsub = nsub;
        cj.nparts = (u32)nparts;
        kh_launch_skm_pack_compact(cj, st);
    }
    c->prof_end();
    HIPCHK(hipGetLastError());
    std::vector<u32> h(ctl_bytes / 4);
    HIPCHK(hipMemcpyAsync(h.data(), d_ctl.b->p, ctl_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h[KH_SKM_XCTL_ERR] & KH_ERR_ORDER) return kh_fail(KH_E_INTERNAL, "kh_skm_pack: a record carried a tag above 31");
    if (h[KH_SKM_XCTL_ERR] & KH_ERR_CAPACITY) {
        if (loc) return KH_OK;
        return kh_fail(KH_E_CAPACITY, "kh_skm_pack: a slot or a part overflowed");
    }
    for (int p = 0; p < nparts; ++p) {   // (with several cursors per part: the records, which then lie with gaps)
        part_n[p] = 0;
        for (u32 q = 0; q < nsub; ++q) part_n[p] += h[KH_SKM_XCTL_CURSORS + (size_t)p * nsub + q];
    }
    if (loc) {
        memcpy(loc->dup, reinterpret_cast<const u8*>(h.data()) + off_dup, 8 * 32);
        loc->done = true;
    }
    return KH_OK;
}
extern "C" int kh_skm_pack(kh_ctx* c, int nseq, const uint8_t* const* seqs, const uint64_t* lens, int on_device,
                           const int* tag_of, int k, uint32_t nslots, int nparts, uint64_t part_cap, void* rec_out,
                           uint32_t* mask_out, uint32_t* count_out, uint32_t* off_out, uint64_t* part_n) {
    return skm_pack_impl(c, nseq, seqs, lens, on_device, tag_of, k, nslots, nparts, part_cap, rec_out, mask_out, count_out, off_out,
                         part_n, nullptr);
}

// The one-GPU use of kh_skm_phased_histogram (exp1_big_group_skm): the pieces are the phases of one group.
struct SkmPhases {
    std::vector<u32> row, join;   // per piece: its phase (the row of `dup` it counts into), "the next piece goes on in the same phase"
    u32 share_q8 = 256;           // share of a piece's instances that are new to its phase, x 256
    std::vector<u64> dup;         // out [pieces][32]: repeats under one tag
    bool done = false;            // an overfilled table: false instead of an error
};
static int skm_phased_impl(kh_ctx* c, int k, int npieces, const void* const* recs, const uint32_t* const* masks,
                           const uint32_t* const* counts, const uint32_t* const* offs, uint32_t nslots, uint32_t cs,
                           uint64_t* hist, uint32_t hist_len, SkmPhases* ph) {
    if (ph) ph->done = false;
    if (!c || npieces < 1 || !recs || !masks || !counts || !offs || !hist || hist_len < 2 || cs < 1)
        return kh_fail(KH_E_ARG, "kh_skm_phased_histogram: bad argument");
    if (!skm_exchange_k(k)) return kh_fail(KH_E_ARG, "the exchange form takes k = %d .. %d", KH_SKM_MIN_K, KH_SKM_MAX_K);
    HIPCHK(hipSetDevice(c->dev));
    hipStream_t st = c->st;
    const size_t off_pieces = 64, off_hist = (off_pieces + sizeof(KhSkmPiece) * (size_t)npieces + 63) & ~(size_t)63;
    const size_t off_pdup = off_hist + 8 * (size_t)hist_len, ws_bytes = off_pdup + (ph ? 8 * 32 * (size_t)npieces : 0);
    Tmp d_ws;
    TMP_ALLOC(d_ws, c, ws_bytes);
    std::vector<u8> up(off_hist, 0);
    KhSkmPiece* hp = reinterpret_cast<KhSkmPiece*>(up.data() + off_pieces);
    for (int i = 0; i < npieces; ++i) {
        hp[i].rec = static_cast<const uint4*>(recs[i]);
        hp[i].mask = masks[i];
        hp[i].count = counts[i];
        hp[i].off = offs[i];
        hp[i].dup_row = ph ? ph->row[i] : (u32)i;
        hp[i].join_next = ph ? ph->join[i] : 0u;
    }
    HIPCHK(hipMemsetAsync(d_ws.b->p, 0, ws_bytes, st));
    HIPCHK(hipMemcpyAsync(d_ws.b->p, up.data(), off_hist, hipMemcpyHostToDevice, st));
    KhSkmPhasedJob job;
    job.pieces = reinterpret_cast<const KhSkmPiece*>(d_ws.as<u8>() + off_pieces);
    job.hist = reinterpret_cast<unsigned long long*>(d_ws.as<u8>() + off_hist);
    job.ctl = d_ws.as<u32>();
    job.dup = ph ? reinterpret_cast<unsigned long long*>(d_ws.as<u8>() + off_pdup) : nullptr;
    job.npieces = (u32)npieces;
    job.share_q8 = std::min<u32>(256, std::max<u32>(1, ph ? ph->share_q8 : 256u));
    job.nslots = nslots;
    job.hist_len = hist_len;
    job.cs = cs;
    job.k = k;
    c->prof_begin(KC_SKM_PHASED);
    kh_launch_skm_phased(job, std::min<u32>(std::max<u32>(1, nslots), 2u * (u32)std::max(1, c->cus)), st);
    c->prof_end();
    HIPCHK(hipGetLastError());
    u32 h_ctl[4];
    HIPCHK(hipMemcpyAsync(h_ctl, d_ws.b->p, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hist, d_ws.as<u8>() + off_hist, 8 * (size_t)hist_len, hipMemcpyDeviceToHost, st));
    if (ph) {
        ph->dup.assign(32 * (size_t)npieces, 0);
        HIPCHK(hipMemcpyAsync(ph->dup.data(), d_ws.as<u8>() + off_pdup, 8 * 32 * (size_t)npieces, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    if (h_ctl[KH_SKM_XCTL_ERR] & KH_ERR_CAPACITY) {
        if (ph) return KH_OK;
        return kh_fail(KH_E_CAPACITY, "kh_skm_phased_histogram: a slot held more k-mers than its table");
    }
    c->stat.setops++;
    if (ph) ph->done = true;
    return KH_OK;
}
extern "C" int kh_skm_phased_histogram(kh_ctx* c, int k, int npieces, const void* const* recs, const uint32_t* const* masks,
                                       const uint32_t* const* counts, const uint32_t* const* offs, uint32_t nslots, uint32_t cs,
                                       uint64_t* hist, uint32_t hist_len) {
    return skm_phased_impl(c, k, npieces, recs, masks, counts, offs, nslots, cs, hist, hist_len, nullptr);
}

// One group of more than 64 genomes in the super-k-mer form (one-word keys): sub-batches of up to 32 genomes, each
// turned into records tagged with the genome's number in the sub-batch, identical records merged (k_skm_pack, one
// part); the sub-batches are the PHASES of one phased union (k_skm_phased): the counter of an entry ends as "in how
// many genomes of the group", which is the group's step_4 histogram.  Distinct k-mers of a genome: its instances minus
// the repeats under its tag (whole records at the merge, single k-mers at the insertion).  *done == false: the
// caller takes the key-array sub-batches.
static int exp1_big_group_skm(kh_ctx* c, int n, const uint8_t* const* seqs, const uint64_t* lens, int on_device, int k, u32 cs,
                              uint64_t* whist, u32 hist_len, uint64_t* dist /* [n] or null */, bool* done) {
    *done = false;
    if (!skm_exchange_k(k) || getenv("KHOICE_NO_SKM") || getenv("KHOICE_NO_SKM_PHASED") || !whist) return KH_OK;
    constexpr int SUB = 32;
    const int P = (n + SUB - 1) / SUB;
    if (P > (int)KH_SKM_PHASED_MAX_DUP_PIECES) return KH_OK;
    std::vector<int> first(P + 1, 0);
    for (int p = 0; p < P; ++p) first[p + 1] = first[p] + (n - first[p] + (P - p) - 1) / (P - p);   // balanced sizes
    u64 pos_max = 0;
    std::vector<u64> pos(P, 0);
    for (int p = 0; p < P; ++p) {
        pos[p] = kmer_positions(first[p + 1] - first[p], lens + first[p], k);
        pos_max = std::max(pos_max, pos[p]);
    }
    if (!pos_max) return KH_OK;
    u64 ns = 0;
    double per_kmer = 0;
    const bool dbg = getenv("KHOICE_SKM_DEBUG") != nullptr;
    // How much the sub-batches of a group share decides how large a slot may be: its table holds one sub-batch's k-mers
    // plus what each further one adds (`novelty` of its own).  Measured: the synthetic genomes (1 % divergence from one
    // ancestor, independent per genome) add 0.7 — with 0.3 assumed a table overfilled and the repeated launch cost more
    // than the 2.5 x larger slots saved (12.1 -> 14.0 ms) — so the default assumes unrelated sub-batches (1.0); real
    // collections with a tree-like history share more: KHOICE_SKM_PHASED_NOVELTY (an overfilled table is caught and the
    // launch repeated with rounds sized for unrelated pieces).
    double novelty = 1.0;
    if (const char* e = getenv("KHOICE_SKM_PHASED_NOVELTY")) novelty = std::min(1.0, std::max(0.05, atof(e)));
    const double eff_parts = 1.0 + novelty * (double)(P - 1);
    const u32 share_q8 = (u32)std::min(256.0, std::ceil(256.0 * eff_parts / (double)P));
    if (!skm_exchange_geometry(k, pos_max, P, (u32)SUB, &ns, &per_kmer, eff_parts)) {
        if (dbg) fprintf(stderr, "[skm phased] %d genomes in %d phases: no geometry for %llu positions per phase\n", n, P, (unsigned long long)pos_max);
        return KH_OK;
    }
    const u32 nslots = (u32)ns;
    if (dbg) fprintf(stderr, "[skm phased] %d genomes in %d phases, %u slots, %.0f positions per slot and phase\n", n, P, nslots, (double)pos_max / nslots);
    HIPCHK(hipSetDevice(c->dev));
    std::vector<std::unique_ptr<Tmp>> bufs;
    std::vector<const void*> recs;
    std::vector<const uint32_t*> masks, counts, offs;
    SkmPhases ph;
    auto add_piece = [&](const u8* b, size_t off_mask, size_t off_count, size_t off_off, u32 row, u32 join) {
        recs.push_back(b);
        masks.push_back(reinterpret_cast<const u32*>(b + off_mask));
        counts.push_back(reinterpret_cast<const u32*>(b + off_count));
        offs.push_back(reinterpret_cast<const u32*>(b + off_off));
        ph.row.push_back(row);
        ph.join.push_back(join);
    };
    std::vector<u64> inst_all(n, 0), dup_all(n, 0);
    hipStream_t st = c->st;
    for (int p = 0; p < P; ++p) {
        const int m = first[p + 1] - first[p];
        const u64 cap = skm_part_cap(pos[p], per_kmer, 1);
        const size_t off_mask = 16 * (size_t)cap, off_count = off_mask + 4 * (size_t)cap, off_off = off_count + 4 * (size_t)((nslots + 3) & ~3u),
                     bytes = off_off + 4 * (size_t)((nslots + 3) & ~3u);
        bufs.emplace_back(new Tmp);
        TMP_ALLOC(*bufs.back(), c, bytes);
        u8* base = bufs.back()->as<u8>();
        std::vector<int> tag(m);
        for (int j = 0; j < m; ++j) tag[j] = j;
        u64 part_n = 0;
        SkmPackLocal loc;
        KHCHK(skm_pack_impl(c, m, seqs + first[p], lens + first[p], on_device, tag.data(), k, nslots, 1, cap, base,
                            reinterpret_cast<u32*>(base + off_mask), reinterpret_cast<u32*>(base + off_count),
                            reinterpret_cast<u32*>(base + off_off), &part_n, &loc));
        if (!loc.done) {
            if (dbg) fprintf(stderr, "[skm phased] phase %d: the records did not fit\n", p);
            return KH_OK;
        }
        if (dbg) fprintf(stderr, "[skm phased] phase %d: %llu records travel (cap %llu), %u on the side list\n", p, (unsigned long long)part_n,
                         (unsigned long long)cap, loc.spill_n);
        add_piece(base, off_mask, off_count, off_off, (u32)p, 0);
        for (int j = 0; j < m; ++j) { inst_all[first[p] + j] = loc.inst[j]; dup_all[first[p] + j] = loc.dup[j]; }
        if (loc.spill_n) {
            // Overfull slots (low-complexity sequence): what the regions could not hold is on the side list, unmerged and
            // in no order.  It joins the sub-batch's phase as extra pieces — sorted by slot on the host (rare, small),
            // at most 1024 records of a slot per piece.
            const u32 ns = loc.spill_n;
            std::vector<uint4> hrec(ns);
            std::vector<u32> hslot(ns), order(ns);
            HIPCHK(hipMemcpyAsync(hrec.data(), loc.spill.b->p, 16 * (size_t)ns, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(hslot.data(), static_cast<const u8*>(loc.spill.b->p) + 16 * (size_t)SkmRun::spill_cap, 4 * (size_t)ns,
                                  hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            for (u32 i = 0; i < ns; ++i) {
                order[i] = i;
                if (hslot[i] >= nslots) return kh_fail(KH_E_INTERNAL, "side list: slot %u of %u", hslot[i], nslots);
            }
            std::stable_sort(order.begin(), order.end(), [&](u32 a, u32 b) { return hslot[a] < hslot[b]; });
            std::vector<u32> run(nslots, 0);
            u32 longest = 0;
            for (u32 i = 0; i < ns; ++i) longest = std::max(longest, ++run[hslot[i]]);
            const u32 extra = (longest + 1023u) / 1024u;
            ph.join.back() = 1;
            for (u32 e = 0; e < extra; ++e) {
                std::vector<uint4> prec;
                std::vector<u32> pmask, pcount(nslots, 0), poff(nslots, 0);
                for (u32 i = 0; i < ns;) {   // the sorted list, a slot's run at a time
                    const u32 sl = hslot[order[i]], len = run[sl];
                    const u32 lo = std::min(len, e * 1024u), hi = std::min(len, (e + 1) * 1024u);
                    poff[sl] = (u32)prec.size();
                    pcount[sl] = hi - lo;
                    for (u32 j = lo; j < hi; ++j) {
                        const uint4 r = hrec[order[i + j]];
                        prec.push_back(r);
                        pmask.push_back(1u << (SkmRec1::tag(r.w) & 31u));   // (tags of the exchange form are below 32)
                    }
                    i += len;
                }
                const size_t nrec_e = std::max<size_t>(1, prec.size());
                const size_t e_mask = 16 * nrec_e, e_count = e_mask + ((4 * nrec_e + 15) & ~(size_t)15), e_off = e_count + 4 * (size_t)((nslots + 3) & ~3u),
                             e_bytes = e_off + 4 * (size_t)((nslots + 3) & ~3u);
                bufs.emplace_back(new Tmp);
                TMP_ALLOC(*bufs.back(), c, e_bytes);
                u8* eb = bufs.back()->as<u8>();
                if (!prec.empty()) {
                    HIPCHK(hipMemcpyAsync(eb, prec.data(), 16 * prec.size(), hipMemcpyHostToDevice, st));
                    HIPCHK(hipMemcpyAsync(eb + e_mask, pmask.data(), 4 * pmask.size(), hipMemcpyHostToDevice, st));
                }
                HIPCHK(hipMemcpyAsync(eb + e_count, pcount.data(), 4 * (size_t)nslots, hipMemcpyHostToDevice, st));
                HIPCHK(hipMemcpyAsync(eb + e_off, poff.data(), 4 * (size_t)nslots, hipMemcpyHostToDevice, st));
                HIPCHK(hipStreamSynchronize(st));   // (the host vectors go out of scope)
                add_piece(eb, e_mask, e_count, e_off, (u32)p, e + 1 < extra ? 1u : 0u);
            }
            c->stat.big_slots += (u64)std::count_if(run.begin(), run.end(), [](u32 v) { return v != 0; });
        }
    }
    std::vector<u64> hist(hist_len, 0);
    ph.share_q8 = share_q8;
    KHCHK(skm_phased_impl(c, k, (int)recs.size(), recs.data(), masks.data(), counts.data(), offs.data(), nslots, cs, hist.data(), hist_len, &ph));
    if (!ph.done && share_q8 < 256) {   // a table overfilled: the genomes share less than assumed — rounds for unrelated pieces
        if (dbg) fprintf(stderr, "[skm phased] a table overfilled with rounds sized for shared k-mers: once more\n");
        c->stat.retries++;
        ph.share_q8 = 256;
        KHCHK(skm_phased_impl(c, k, (int)recs.size(), recs.data(), masks.data(), counts.data(), offs.data(), nslots, cs, hist.data(), hist_len, &ph));
    }
    if (!ph.done) {
        if (dbg) fprintf(stderr, "[skm phased] the phased union overflowed\n");
        return KH_OK;
    }
    memcpy(whist, hist.data(), 8 * (size_t)hist_len);
    u64 bases = 0, isum = 0, dsum = 0;
    for (int p = 0; p < P; ++p)
        for (int i = first[p]; i < first[p + 1]; ++i) {
            const u64 d = inst_all[i] - dup_all[i] - ph.dup[(size_t)p * 32 + (i - first[p])];
            if (dist) dist[i] = d;
            bases += lens[i]; isum += inst_all[i]; dsum += d;
        }
    c->stat.bases += bases;
    c->stat.builds += n;
    c->stat.kmers += isum;
    c->stat.distinct += dsum;
    c->stat.setop_in += dsum;
    *done = true;
    return KH_OK;
}

// What the presence-bitmap forms (exp1_bmp .. exp4_bmp, exp6_bmp) share: the switches, the geometry of the build, the tables of
// splits and operands, the copy-in of the texts, and the run that strings them together (BmpRun).
static bool bmp_form_k(int k) {
    int max_k = KH_BMP_MAX_K;
    if (const char* e = getenv("KHOICE_BMP_MAX_K")) max_k = std::min(KH_BMP_INST_MAX_K, atoi(e));
    // (KHOICE_NO_SKM: "the key arrays, please"; KHOICE_SKM_MIN_K lowered to this k: the super-k-mer form keeps it)
    return !(k > max_k || getenv("KHOICE_NO_BMP") || getenv("KHOICE_NO_SKM") || skm_form_k(k));
}
struct BmpStage {
    u64 nwords = 0, nsplits = 0, bases = 0;
    u32 range_bits = 0, nranges = 0, tile_pos = 0;
    u32 rwaves = 0, rgrid = 0;            // launch shape of the read-out
    std::vector<KhBmpSplit> splits;       // (seq: filled in by BmpRun::upload)
    std::vector<KhBmpOp> ops;
};
// nops operands (seqs / lens in operand order).  extra_rows: further bitmaps of nwords words the caller keeps beside
// the partial ones, under the same budget.  *fits == false: the form declines.
static int bmp_plan(kh_ctx* c, int k, int nops, const uint64_t* lens, u64 extra_rows, BmpStage* s, bool* fits) {
    *fits = false;
    // ---- geometry: ranges of the code space, tiles, splits
    const u64 nwords = k >= 3 ? 1ull << (2 * k - 6) : 1;
    u32 range_bits = KH_BMP_RANGE_BITS;
    if (const char* e = getenv("KHOICE_BMP_RANGE_BITS")) range_bits = (u32)std::min(20, std::max(16, atoi(e)));   // experiments
    range_bits = std::min<u32>(range_bits, (u32)std::max(6, 2 * k));
    const u32 nranges = (u32)((nwords * 64) >> range_bits);
    u32 tile_pos = KH_BMP_TILE;
    if (const char* e = getenv("KHOICE_BMP_TILE_POS"))
        tile_pos = std::min<u32>(KH_BMP_TILE, std::max<u32>(16, (u32)strtoul(e, nullptr, 10) & ~15u));
    u64 bases = 0, maxpos = 0;
    const u64 positions = kmer_positions(nops, lens, k, &bases);
    for (int i = 0; i < nops; ++i) maxpos = std::max<u64>(maxpos, lens[i] >= (u64)k ? lens[i] - k + 1 : 0);
    // Splits: genomes x splits x ranges is a small multiple of the CU count, but a split is long enough to pay for the
    // words of its range that its workgroup clears and stores (one bit per position would be the break-even)
    const u64 want_wgs = 4ull * (u64)std::max(1, c->cus);
    const u64 want_splits = std::max<u64>(1, want_wgs / nranges);
    u64 split_pos = std::max<u64>((positions + want_splits - 1) / want_splits, std::max<u64>(tile_pos, (1ull << range_bits) / 16));
    if (const char* e = getenv("KHOICE_BMP_SPLIT_POS")) split_pos = std::max<u64>(16, strtoull(e, nullptr, 10));
    split_pos = (split_pos + 15) & ~15ull;
    auto count_splits = [&](u64 sp) {
        u64 n = 0;
        for (int i = 0; i < nops; ++i) {
            const u64 npos = lens[i] >= (u64)k ? lens[i] - k + 1 : 0;
            n += std::max<u64>(1, (npos + sp - 1) / sp);   // a genome without k-mers: one split, all zeros
        }
        return n;
    };
    HIPCHK(hipSetDevice(c->dev));
    u64 budget = 1ull << 30;
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = (free_b + c->pool.cached_bytes) / 4;
    }
    if (const char* e = getenv("KHOICE_BMP_MAX_BYTES")) budget = strtoull(e, nullptr, 10);
    u64 nsplits = count_splits(split_pos);
    while ((nsplits + extra_rows) * nwords * 8 > budget && split_pos < maxpos) {   // fewer, longer splits: fewer partial bitmaps
        split_pos *= 2;
        nsplits = count_splits(split_pos);
    }
    if ((nsplits + extra_rows) * nwords * 8 > budget || nsplits * nranges > 0x7fffffffull) return KH_OK;
    const size_t lds_build = kh_bmp_build_lds_bytes(range_bits, tile_pos);
    if (lds_build > 160u * 1024u) return KH_OK;
    if (getenv("KHOICE_BMP_DEBUG"))
        fprintf(stderr, "[bmp] k=%d range_bits=%u R=%u tile_pos=%u split_pos=%llu splits=%llu workgroups=%llu bitmap_bytes=%llu\n", k,
                range_bits, nranges, tile_pos, (unsigned long long)split_pos, (unsigned long long)nsplits,
                (unsigned long long)(nsplits * nranges), (unsigned long long)((nsplits + extra_rows) * nwords * 8));

    // ---- tables: splits and operands
    s->nwords = nwords; s->nsplits = nsplits; s->bases = bases;
    s->range_bits = range_bits; s->nranges = nranges; s->tile_pos = tile_pos;
    s->ops.resize(nops);
    s->splits.reserve(nsplits);
    for (int i = 0; i < nops; ++i) {
        const u64 len = lens[i], npos = len >= (u64)k ? len - k + 1 : 0;
        s->ops[i].split0 = (u32)s->splits.size();
        u64 p0 = 0;
        do {
            const u64 p1 = std::min(npos, p0 + split_pos);
            s->splits.push_back(KhBmpSplit{nullptr, len, p0, p1, (u32)i, 0});
            p0 = p1;
        } while (p0 < npos);
        s->ops[i].nsplits = (u32)s->splits.size() - s->ops[i].split0;
    }
    // the read-out: a wave per 64 words and genome; where the words alone leave most of the chip idle (k <= 10: at
    // most 256 blocks of 64 words) sixteen genomes are in flight per block, else four
    const u64 rblocks = (nwords + 63) / 64;
    s->rwaves = rblocks <= 256 ? 16u : 4u;
    s->rgrid = (u32)std::min<u64>(rblocks, 8ull * (u64)std::max(1, c->cus));
    *fits = true;
    return KH_OK;
}
// The operands of a bitmap run: the genomes in group-major order (within a group in the caller's order), then the
// pivots — with pivot_group, each behind the genomes of the group it was held out of.
struct BmpOperands {
    std::vector<const uint8_t*> seq;
    std::vector<uint64_t> len;
    std::vector<int> op_of_seq, op_of_pivot;
    std::vector<u32> first, size;         // per group: its first operand, its genomes
};
static BmpOperands bmp_operands(int nseq, const uint8_t* const* seqs, const uint64_t* lens, const int* group_of, int ngroups,
                                int npiv = 0, const uint8_t* const* pivot_seqs = nullptr, const uint64_t* pivot_lens = nullptr,
                                const int* pivot_group = nullptr) {
    BmpOperands o;
    o.seq.resize(nseq + npiv);
    o.len.resize(nseq + npiv);
    o.op_of_seq.resize(nseq);
    o.op_of_pivot.resize(npiv);
    o.first.resize(ngroups);
    o.size.assign(ngroups, 0);
    std::vector<u32> held(ngroups, 0), at(ngroups);
    for (int i = 0; i < nseq; ++i) o.size[group_of[i]]++;
    for (int p = 0; p < npiv && pivot_group; ++p) held[pivot_group[p]]++;
    u32 next = 0;
    for (int g = 0; g < ngroups; ++g) {
        o.first[g] = at[g] = next;
        next += o.size[g] + held[g];
    }
    auto place = [&](u32 op, const uint8_t* s, uint64_t l) {
        o.seq[op] = s;
        o.len[op] = l;
        return (int)op;
    };
    for (int i = 0; i < nseq; ++i) o.op_of_seq[i] = place(at[group_of[i]]++, seqs[i], lens[i]);
    for (int p = 0; p < npiv; ++p) o.op_of_pivot[p] = place(pivot_group ? at[pivot_group[p]]++ : next++, pivot_seqs[p], pivot_lens[p]);
    return o;
}
// The groups' table entries of types 1 and 4: one bin per count 0 .. size of every group, one group's bins behind the
// other's; *nbins: the bins in all.  false: a group has more genomes than a counter takes.
static bool bmp_group_table(const BmpOperands& o, std::vector<KhBmpGroup>* groups, u64* nbins) {
    groups->resize(o.size.size());
    *nbins = 0;
    for (size_t g = 0; g < o.size.size(); ++g) {
        if (o.size[g] > KH_BMP_MAX_COUNT) return false;
        (*groups)[g] = KhBmpGroup{o.first[g], o.size[g], (u32)*nbins, 0};
        *nbins += o.size[g] + 1;
    }
    return true;
}
// One run of a presence-bitmap form, what exp1_bmp .. exp4_bmp and exp6_bmp do alike.  In this order: plan(); layout(); table() for
// every table of the form's own; upload(); build(); the form's launches (timed_launch); download(); then bins(), inst()
// and account().
// Workspace: [hist: blocks x reps x nb u64][inst: nops u64] (zeroed, read back) [splits][ops][the form's tables] (one
// upload, zero where a table's alignment leaves a gap)
struct BmpRun {
    kh_ctx* c;
    int k, on_device;
    const BmpOperands& o;
    BmpStage s;
    u32 nb = 0, reps = 0;                 // bins and counters of a block of replicas (the largest launch's), replicas
    size_t hist_stride = 0, off_inst = 0, off_splits = 0, off_ops = 0, ws_bytes = 0;
    struct Table { size_t off; const void* src; size_t bytes; };
    std::vector<Table> tables;
    TextStage texts;
    Tmp d_ws, d_partial;
    Pinned pin;
    u8 *h_up = nullptr, *h_down = nullptr;

    BmpRun(kh_ctx* ctx, int k_, int on_dev, const BmpOperands& ops) : c(ctx), k(k_), on_device(on_dev), o(ops), pin{ctx} {}
    int nops() const { return (int)o.seq.size(); }
    static u32 reps_max(u32 nb) { return std::max<u32>(1, std::min<u32>(64, 65536u / nb)); }
    // *fits == false: the form declines
    int plan(u64 extra_rows, bool* fits) { return bmp_plan(c, k, nops(), o.len.data(), extra_rows, &s, fits); }
    void layout(u32 blocks, u32 nb_of_block) {
        nb = nb_of_block;
        reps = std::min(s.rgrid, reps_max(nb));
        hist_stride = 8 * (size_t)reps * nb;
        off_inst = hist_stride * blocks;
        ws_bytes = off_inst + 8 * (size_t)nops();
        off_splits = table(s.splits);     // (their texts are filled in by upload())
        off_ops = table(s.ops);
    }
    // a table behind the ones laid out so far; returns its offset in the workspace (dev()).  v stays until upload().
    template <class T> size_t table(const std::vector<T>& v) {
        const size_t off = (ws_bytes + alignof(T) - 1) & ~(alignof(T) - 1);
        tables.push_back(Table{off, v.data(), sizeof(T) * v.size()});
        ws_bytes = off + sizeof(T) * v.size();
        return off;
    }
    // the device memory, the texts copied in, the zeroed region zeroed and the tables uploaded; `also` runs among the copies
    template <class F> int upload(F also) {
        TMP_ALLOC(d_ws, c, ws_bytes);
        TMP_ALLOC(d_partial, c, (size_t)(s.nsplits * s.nwords * 8));
        const size_t up_bytes = ws_bytes - off_splits;
        PIN_ALLOC(pin, up_bytes + off_splits + 64);
        h_up = static_cast<u8*>(pin.p);
        h_down = h_up + ((up_bytes + 63) & ~(size_t)63);
        c->prof_begin(KC_COPY_IN);
        KHCHK(texts.copy_in(c, nops(), o.seq.data(), o.len.data(), on_device));
        for (KhBmpSplit& sp : s.splits) sp.seq = texts.dev[sp.op];   // every split learns its text
        memset(h_up, 0, up_bytes);
        for (const Table& t : tables)
            if (t.bytes) memcpy(h_up + (t.off - off_splits), t.src, t.bytes);
        HIPCHK(hipMemsetAsync(d_ws.b->p, 0, off_splits, c->st));
        KHCHK(also());
        HIPCHK(hipMemcpyAsync(d_ws.as<u8>() + off_splits, h_up, up_bytes, hipMemcpyHostToDevice, c->st));
        c->prof_end();
        return KH_OK;
    }
    int upload() { return upload([] { return (int)KH_OK; }); }
    template <class T> T* dev(size_t off) const { return reinterpret_cast<T*>(d_ws.as<u8>() + off); }
    const KhBmpOp* ops() const { return dev<const KhBmpOp>(off_ops); }
    unsigned long long* hist(u32 block) const { return dev<unsigned long long>(hist_stride * block); }
    KhBmpJob build_job() const {
        KhBmpJob job{};
        job.splits = dev<const KhBmpSplit>(off_splits);
        job.partial = d_partial.as<u64>();
        job.inst = dev<unsigned long long>(off_inst);
        job.nwords = s.nwords;
        job.tile_pos = s.tile_pos;
        job.range_bits = s.range_bits; job.nranges = s.nranges;
        job.nops = (u32)nops();
        job.k = k;
        return job;
    }
    int build() {
        const KhBmpJob job = build_job();
        return timed_launch(c, KC_BMP_BUILD, [&] { kh_launch_bmp_build(job, (u32)s.nsplits, c->st); });
    }
    int download() {
        HIPCHK(hipMemcpyAsync(h_down, d_ws.b->p, off_splits, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
        return KH_OK;
    }
    const u64* inst() const { return reinterpret_cast<const u64*>(h_down + off_inst); }   // [nops] valid positions
    // the replicas of a block summed; nb_of_launch: the bins and counters of the launch that filled it
    void bins(u32 block, u32 nb_of_launch, std::vector<u64>* out) const {
        const u64* h = reinterpret_cast<const u64*>(h_down + hist_stride * block);
        out->assign(nb_of_launch, 0);
        for (u32 r = 0; r < reps; ++r)
            for (u32 b = 0; b < nb_of_launch; ++b) (*out)[b] += h[(size_t)r * nb_of_launch + b];
    }
    // the operands' distinct k-mers, counters first_counter .. of `bins`: their sum; every sequence's into per_seq (or null)
    u64 distinct(const std::vector<u64>& bins, u64 first_counter, uint64_t* per_seq) const {
        u64 sum = 0;
        for (int op = 0; op < nops(); ++op) sum += bins[first_counter + op];
        for (size_t i = 0; i < o.op_of_seq.size() && per_seq; ++i) per_seq[i] = bins[first_counter + o.op_of_seq[i]];
        return sum;
    }
    // distinct: the operands' distinct k-mers summed; setop_out: what the form counts as its set operations' output
    void account(u64 distinct, u64 setop_out) const {
        u64 kmers = 0;
        for (int i = 0; i < nops(); ++i) kmers += inst()[i];
        c->stat.bases += s.bases;
        c->stat.builds += nops();
        c->stat.kmers += kmers;
        c->stat.distinct += distinct;
        c->stat.setop_in += distinct;
        c->stat.setop_out += setop_out;
        c->stat.setops++;
    }
};
// The bin of a count in a histogram of a -cs{cs} union: counts saturate at cs and at the last bin.
static u32 count_bin(u32 cnt, u32 cs, u32 hist_len) { return std::min(std::min(cnt, cs), hist_len - 1); }
// The bin of pivot k-mers that v genomes hold, in the histogram of `intersect -ocsum` with the -cs{cs} union: the
// pivot's own 1 is added to the union's saturated counter, and the sum saturates again.
static u32 ocsum_bin(u32 v, u32 cs, u32 hist_len) { return std::min(std::min(1 + std::min(v, cs), cs), hist_len - 1); }
// within_hist[g]: the bins of group g's counter (bins[bin0 + cnt], cnt = 1 .. size) folded
static void fold_within(const std::vector<KhBmpGroup>& groups, const std::vector<u64>& bins, u32 cs, uint64_t* within_hist, u32 hist_len) {
    if (!within_hist) return;
    memset(within_hist, 0, 8 * groups.size() * hist_len);
    for (size_t g = 0; g < groups.size(); ++g)
        for (u32 cnt = 1; cnt <= groups[g].size; ++cnt)
            within_hist[g * hist_len + count_bin(cnt, cs, hist_len)] += bins[groups[g].bin0 + cnt];
}
// What the set forms of types 2-4 do alike.  genomes (and pivots behind them) in one plain batched build:
static int build_plain(kh_ctx* c, int nseq, const uint8_t* const* seqs, const uint64_t* lens, int npiv, const uint8_t* const* pivot_seqs,
                       const uint64_t* pivot_lens, int on_device, int k, SetBag* plain) {
    std::vector<const uint8_t*> s(seqs, seqs + nseq);
    std::vector<uint64_t> l(lens, lens + nseq);
    s.insert(s.end(), pivot_seqs, pivot_seqs + npiv);
    l.insert(l.end(), pivot_lens, pivot_lens + npiv);
    plain->v.assign(nseq + npiv, nullptr);
    return kh_build_batch(c, nseq + npiv, s.data(), l.data(), on_device, k, 1, KH_NO_MAX, KH_KMC_DEFAULT_CS, 0, plain->v.data());
}
// unions->v[g]: the -cs{cs} union of group g's genomes (plain[i], i < nseq); hist: [ngroups][hist_len] the unions'
// histograms, or null
static int group_unions(kh_ctx* c, kh_set* const* plain, int nseq, const int* group_of, int ngroups, u32 cs, SetBag* unions,
                        uint64_t* hist, u32 hist_len) {
    unions->v.assign(ngroups, nullptr);
    for (int g = 0; g < ngroups; ++g) {
        std::vector<const kh_set*> members;
        for (int i = 0; i < nseq; ++i)
            if (group_of[i] == g) members.push_back(plain[i]);
        KHCHK(kh_union_sum(c, members.data(), (int)members.size(), cs, &unions->v[g], hist ? hist + (size_t)g * hist_len : nullptr,
                           hist ? hist_len : 0));
    }
    return KH_OK;
}
// ones->v[g]: unions.v[g] with every counter 1 (`set_counts 1`)
static int group_ones(kh_ctx* c, const SetBag& unions, SetBag* ones) {
    ones->v.assign(unions.v.size(), nullptr);
    for (size_t g = 0; g < unions.v.size(); ++g) KHCHK(kh_set_counts(c, unions.v[g], 1, &ones->v[g]));
    return KH_OK;
}
// What kh_exp2_run, kh_exp3_run and kh_exp4_run check alike, in the order they check it.  has_pivot_group: the call
// has a pivot_group; pivot_cs: null where the call has none.
static int exp_check_args(const char* who, const kh_ctx* c, int nseq, const void* seqs, const void* lens, const int* group_of, int ngroups,
                          int npivots, const void* pivot_seqs, const void* pivot_lens, bool has_pivot_group, const int* pivot_group,
                          u32 hist_len, int k, u32 cs, const u32* pivot_cs) {
    if (!c || !seqs || !lens || !group_of || nseq <= 0 || ngroups <= 0 || npivots < 0 ||
        (npivots && (!pivot_seqs || !pivot_lens || (has_pivot_group && !pivot_group))))
        return kh_fail(KH_E_ARG, "%s: bad argument", who);
    if (hist_len < 2) return kh_fail(KH_E_ARG, "hist_len must be >= 2");
    KHCHK(check_k(k));
    if (cs < 1) return kh_fail(KH_E_ARG, "cs must be >= 1");
    if (pivot_cs && *pivot_cs < 1) return kh_fail(KH_E_ARG, "pivot_cs must be >= 1");
    std::vector<int> gsize(ngroups, 0);
    for (int i = 0; i < nseq; ++i) {
        if (group_of[i] < 0 || group_of[i] >= ngroups)
            return kh_fail(KH_E_ARG, "group_of[%d]=%d outside [0,%d)", i, group_of[i], ngroups);
        gsize[group_of[i]]++;
    }
    for (int g = 0; g < ngroups; ++g)
        if (!gsize[g]) return kh_fail(KH_E_ARG, "group %d has no sequences", g);
    for (int p = 0; p < npivots && has_pivot_group; ++p)
        if (pivot_group[p] < 0 || pivot_group[p] >= ngroups)
            return kh_fail(KH_E_ARG, "pivot_group[%d]=%d outside [0,%d)", p, pivot_group[p], ngroups);
    return KH_OK;
}
// The presence-bitmap form of the fused path (kh_bmp.hip) for k <= KH_BMP_MAX_K, histograms and distinct counts only: a
// k-mer is a number below 4^k, so "which genomes hold it" is one bit per genome in a directly addressed bitmap.
// k_bmp_build turns every split of a genome into a partial bitmap, k_bmp_readout counts over them with bit-sliced
// counters.  There is no genome mask: groups of up to 1023 genomes and up to 1023 groups are one pass.  *done == false:
// the form does not apply (nothing was launched, no retry is counted) — the caller goes on to the other forms.
static int exp1_bmp(kh_ctx* c, const Exp1In& in, uint64_t* within_hist, uint64_t* across_hist, uint64_t* distinct_per_seq,
                    bool* done) {
    *done = false;
    const int k = in.k, nseq = in.nseq, ngroups = in.ngroups;
    if (!bmp_form_k(k) || (u32)ngroups > KH_BMP_MAX_COUNT) return KH_OK;
    const BmpOperands o = bmp_operands(nseq, in.seqs, in.lens, in.group_of, ngroups);
    // ---- bins: per group one per count of its genomes, then one per count of groups (across)
    std::vector<KhBmpGroup> groups;
    u64 nbins = 0;
    if (!bmp_group_table(o, &groups, &nbins)) return KH_OK;
    for (int g = 0; g < ngroups; ++g)
        if (!o.size[g]) return KH_OK;   // (a group without genomes: the general path reports it)
    const u32 abase = (u32)nbins;
    nbins += (u64)ngroups + 1;
    if (nbins > KH_BMP_MAX_BINS) return KH_OK;
    BmpRun run(c, k, in.on_device, o);
    bool fits = false;
    KHCHK(run.plan(0, &fits));
    if (!fits) return KH_OK;
    run.layout(1, (u32)nbins + (u32)nseq);   // the bins, then one distinct counter per operand
    const size_t off_groups = run.table(groups);
    KHCHK(run.upload());
    KHCHK(run.build());
    KhBmpJob job = run.build_job();
    job.ops = run.ops();
    job.groups = run.dev<const KhBmpGroup>(off_groups);
    job.hist = run.hist(0);
    job.ngroups = (u32)ngroups; job.nbins = (u32)nbins; job.abase = abase; job.reps = run.reps;
    KHCHK(timed_launch(c, KC_BMP_READOUT, [&] { kh_launch_bmp_readout(job, run.s.rgrid, run.s.rwaves, c->st); }));
    KHCHK(run.download());

    // ---- the bins folded: counts saturate at cs and at the last bin
    std::vector<u64> bins;
    run.bins(0, run.nb, &bins);
    fold_within(groups, bins, in.cs, within_hist, in.hist_len);
    u64 across_n = 0;
    if (across_hist) memset(across_hist, 0, 8 * (size_t)in.hist_len);
    for (u32 cnt = 1; cnt <= (u32)ngroups; ++cnt) {
        across_n += bins[abase + cnt];
        if (across_hist) across_hist[count_bin(cnt, in.cs, in.hist_len)] += bins[abase + cnt];
    }
    run.account(run.distinct(bins, nbins, distinct_per_seq), across_n);
    *done = true;
    return KH_OK;
}
// The fused form of steps 1-8 (no per-genome / per-group database is handed out): ONE batched build
// in grid mode, ONE tagged union over all genomes, ONE host synchronisation.  *done == false on
// return means "not applicable or a slot overflowed": the caller takes the general path.
static int exp1_fused(kh_ctx* c, int nseq, const uint8_t* const* seqs, const uint64_t* lens, int on_device,
                      const int* group_of, int ngroups, int k, u32 cs, uint64_t* within_hist,
                      uint64_t* across_hist, u32 hist_len, uint64_t* distinct_per_seq, kh_set** across_set,
                      bool* done, u32 nwaves = 1, double s_scale = 1.0, double* want_scale = nullptr, u32 fan_hint = 0) {
    *done = false;
    if (want_scale) *want_scale = 0.0;
    const int W = k <= 32 ? 1 : 2;
    if (nseq > KH_TAG_MAX_OPS || ngroups > KH_TAG_MAX_OPS) return KH_OK;
    TagLayout L;
    KHCHK(tag_layout(&L, nseq, group_of, ngroups, false));
    if (L.nbins > (u32)KH_TAG_MAX_BINS) return KH_OK;
    const u32 mean = k <= 32 ? KH_BUCKET_MEAN_W1 : KH_BUCKET_MEAN_W2;
    std::vector<const uint8_t*> pseq(nseq);
    std::vector<uint64_t> plen(nseq);
    for (int i = 0; i < nseq; ++i) {
        pseq[i] = seqs[L.perm[i]];
        plen[i] = lens[L.perm[i]];
        // longer than one segment's bucket table: the general path cuts such sequences into chunks
        if (lens[L.perm[i]] >= (u64)k && lens[L.perm[i]] - k + 1 > (u64)(KH_MAX_BUCKETS_PER_SEG / 4) * mean) return KH_OK;
    }
    HIPCHK(hipSetDevice(c->dev));
    hipStream_t st = c->st;

    std::vector<u64> bins(L.nbins, 0), dist_acc(nseq, 0);
    const bool emit = across_set != nullptr;
    SetBag wave_sets;   // emitted across-group sets, one per wave (disjoint, ascending key ranges)
    for (u32 wave = 0; wave < nwaves; ++wave) {
    GridBuild gb;
    gb.fan = std::max(L.fan, fan_hint);   // (fan_hint: genomes that are related although every one is a group of its own here)
    gb.wave = wave;
    gb.nwaves = nwaves;
    gb.s_scale = s_scale;
    // one-word keys, nothing emitted: the hash-set kernel; its slot size is a tuning choice
    const bool hash_form = W == 1 && !emit && !getenv("KHOICE_NO_UNION_HASH");
    gb.cap = hash_form ? kh_union_hash_capacity() : (W == 1 ? KH_SORT_CAP_PAY_W1 : KH_SORT_CAP_PAY_W2);
    bool cap_hit = false, again = false;
    {
        const int br = build_once(c, nseq, pseq.data(), plen.data(), on_device, k, 1, KH_NO_MAX, KH_KMC_DEFAULT_CS, 0, mean,
                                  nullptr, &cap_hit, &again, &gb);
        if (br != KH_OK) return br;
    }

    // ---- tagged union queued behind the build
    const u32 nslots = gb.nb * gb.S;
    const u32 grid = nslots;
    const u32 reps = std::min<u32>(256, std::max<u32>(1, grid));
    // workspace: [hist: reps x nbins u64][ctl: 8 u32][out_n u64][ginfo: 64 u32][descriptors: nslots u64 when emitting]
    const size_t hist_words = (size_t)reps * L.nbins;
    const size_t ws_bytes = 8 * hist_words + 32 + 8 + 256 + (emit ? 8 * (size_t)nslots : 0);
    Tmp d_ws;
    TMP_ALLOC(d_ws, c, ws_bytes);
    u8* wsp = d_ws.as<u8>();
    Pinned pin{c};
    // pinned staging: [ginfo upload: 64 u32][hist read-back][ctl + out_n: 40 B][distinct: nseq u64][pass C tail: 64 B][nvalid u64]
    PIN_ALLOC(pin, 256 + 8 * hist_words + 40 + 8 * (size_t)nseq + 64 + 8);
    u32* h_ginfo = static_cast<u32*>(pin.p);
    u64* h_hist = reinterpret_cast<u64*>(h_ginfo + 64);
    u32* h_ctl = reinterpret_cast<u32*>(h_hist + hist_words);
    u64* h_distinct = reinterpret_cast<u64*>(h_ctl + 10);
    u64* h_ctail = h_distinct + nseq;
    u64* h_nvalid = h_ctail + 8;
    L.words(h_ginfo, nullptr, group_of);
    HIPCHK(hipMemsetAsync(wsp, 0, 8 * hist_words + 40, st));
    HIPCHK(hipMemcpyAsync(wsp + 8 * hist_words + 40, h_ginfo, 256, hipMemcpyHostToDevice, st));
    if (emit) HIPCHK(hipMemsetAsync(wsp + 8 * hist_words + 40 + 256, 0, 8 * (size_t)nslots, st));
    DevBuf *okeys = nullptr, *ocnt = nullptr;
    struct OutGuard { DevBuf*& a; DevBuf*& b; ~OutGuard() { buf_unref(a); buf_unref(b); } } og{okeys, ocnt};
    if (emit) {
        okeys = c->buf_alloc(8 * (size_t)W * std::max<u64>(1, gb.key_cap));
        ocnt = c->buf_alloc(4 * std::max<u64>(1, gb.key_cap));
        if (!okeys || !ocnt) return kh_fail(KH_E_NOMEM, "device allocation failed (across-group set)");
    }
    KhTagJob job;
    job.keys = gb.okeys->p;
    job.bstart = reinterpret_cast<const u64*>(gb.bstart->p);
    job.off = reinterpret_cast<const u16*>(gb.off->p);
    job.ginfo = reinterpret_cast<const u32*>(wsp + 8 * hist_words + 40);
    job.hist = reinterpret_cast<unsigned long long*>(wsp);
    job.ctl = reinterpret_cast<u32*>(wsp + 8 * hist_words);
    job.nb = gb.nb; job.S = gb.S; job.nops = (u32)nseq; job.nbins = L.nbins; job.abase = L.abase;
    job.ngroups = (u32)ngroups; job.reps = reps;
    job.nbv = gb.nb * nwaves;
    job.binmul = (1u << 26) / ((KH_FINE_BINS + gb.S - 1) / gb.S);
    job.out_keys = emit ? okeys->p : nullptr;
    job.out_counts = emit ? reinterpret_cast<u32*>(ocnt->p) : nullptr;
    job.desc = emit ? reinterpret_cast<u64*>(wsp + 8 * hist_words + 40 + 256) : nullptr;
    job.out_n = reinterpret_cast<unsigned long long*>(wsp + 8 * hist_words + 32);
#ifdef KH_STAMPS
    Tmp d_stamps;
    TMP_ALLOC(d_stamps, c, 128 * (u64)grid);
    HIPCHK(hipMemsetAsync(d_stamps.b->p, 0, 128 * (u64)grid, st));
    kh_debug_set_stamps(d_stamps.as<u64>());
#endif
    c->prof_begin(KC_UNION_TAGGED);
    if (hash_form) kh_launch_union_hash(job, grid, k, cs, st);
    else kh_launch_union_tagged(W, job, grid, k, cs, st);
    c->prof_end();
    HIPCHK(hipGetLastError());
#ifdef KH_STAMPS
    report_stamps(c, "union_tagged", d_stamps.b, grid);
    kh_debug_set_stamps(nullptr);
#endif
    // ---- one read-back, one wait
    HIPCHK(hipMemcpyAsync(h_hist, wsp, 8 * hist_words + 40, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_distinct, gb.distinct->p, 8 * (size_t)nseq, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_ctail, reinterpret_cast<u64*>(gb.lb->p) + gb.nb_total, 64, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_nvalid, reinterpret_cast<u64*>(gb.bstart->p) + gb.nb_total, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const u32 cerr = reinterpret_cast<const u32*>(h_ctail)[1];   // pass C: [ticket, err]
    const u32 uerr = h_ctl[0];
    if ((cerr | uerr) & (KH_ERR_CAPACITY | KH_ERR_SPIN_TIMEOUT | KH_ERR_ORDER)) {
        c->stat.retries++;
        // a slot of the union held more records than fit (keys shared by many genomes, repeats): the
        // kernel recorded its fullest slot, the caller may try again with that many more sub-ranges
        if (want_scale && !(cerr & KH_ERR_CAPACITY) && (uerr & KH_ERR_CAPACITY) && !(uerr & KH_ERR_ORDER) && h_ctl[1] > gb.cap)
            *want_scale = s_scale * 1.15 * (double)h_ctl[1] / (double)gb.cap;
        return KH_OK;   // otherwise the general path re-plans
    }
    if (wave == 0) { c->stat.bases += gb.bases; c->stat.builds += nseq; }
    c->stat.kmers += *h_nvalid;
    c->stat.setops++;
    u64 dsum = 0;
    for (int i = 0; i < nseq; ++i) {
        dist_acc[i] += h_distinct[i];
        dsum += h_distinct[i];
    }
    c->stat.distinct += dsum;
    c->stat.setop_in += dsum;
    L.add_bins(bins, h_hist, reps);
    if (emit) {
        const u64 n = *reinterpret_cast<const u64*>(h_ctl + 8);
        buf_ref(okeys);
        buf_ref(ocnt);
        wave_sets.v.push_back(make_set(k, n, okeys, 0, ocnt, 0, 1, cs));
    }
    }   // waves
    if (distinct_per_seq)
        for (int i = 0; i < nseq; ++i) distinct_per_seq[L.perm[i]] = dist_acc[i];
    L.fold(c, bins, within_hist, across_hist, hist_len);
    if (across_set) {
        if (wave_sets.v.size() == 1) {
            *across_set = wave_sets.v[0];
            wave_sets.v.clear();
        } else {   // the waves' sets cover disjoint key ranges: their union is their concatenation
            KHCHK(kh_union_sum(c, wave_sets.v.data(), (int)wave_sets.v.size(), cs, across_set, nullptr, 0));
        }
    }
    *done = true;
    return KH_OK;
}
// ---- experiment 1: the forms and their dispatch
// Groups are run in waves that fit a device memory budget.  A base in flight costs ~8W bytes in the partition array +
// 8W (+4) in the output arrays + its share of the group union: budget = 1/64 (W=1) or 1/96 (W=2) of the free HBM, in
// bases.  (Free memory depends on what the pool holds at the time: it is asked again where a plan is made.)
static u64 exp1_wave_bases(kh_ctx* c, int k) {
    u64 budget = 4ull << 30;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
        budget = std::max<u64>(1u << 20, (free_b + c->pool.cached_bytes) / (k <= 32 ? 64 : 96));
    if (const char* e = getenv("KHOICE_WAVE_BASES")) budget = std::max<u64>(1, strtoull(e, nullptr, 10));
    return budget;
}
// a batch whose bases exceed the budget: key-range waves (HBM-spill partitioning of BASELINE
// configs[4]) — every wave re-extracts the batch's bases but keeps one slice of the key space,
// so the memory in flight is 1/waves of the keys and the histograms of the waves add up
static u32 exp1_waves(u64 bases, u64 budget) { return (u32)std::max<u64>(1, (bases + budget - 1) / budget); }

// Some of the caller's sequences as the forms take them, groups numbered from 0; `dist` receives their distinct k-mers,
// scatter() hands them back in the caller's order.
struct SubBatch {
    std::vector<int> idx;                   // the caller's numbers of the sequences
    std::vector<const uint8_t*> seqs;
    std::vector<uint64_t> lens, dist;
    std::vector<int> group;
    int ngroups = 0;
    u64 bases = 0;
    int n() const { return (int)idx.size(); }
    void add(const Exp1In& in, int i, int g) {
        idx.push_back(i);
        seqs.push_back(in.seqs[i]);
        lens.push_back(in.lens[i]);
        dist.push_back(0);
        group.push_back(g);
        bases += in.lens[i];
    }
    Exp1In view(const Exp1In& in) const {   // as the forms take the whole input
        return Exp1In{n(), seqs.data(), lens.data(), in.on_device, group.data(), ngroups, in.k, in.cs, in.hist_len};
    }
    void scatter(uint64_t* distinct_per_seq) const {
        if (distinct_per_seq)
            for (size_t j = 0; j < idx.size(); ++j) distinct_per_seq[idx[j]] = dist[j];
    }
};
static SubBatch groups_batch(const Exp1In& in, int g0, int g1) {   // the sequences of groups [g0, g1)
    SubBatch b;
    b.ngroups = g1 - g0;
    for (int i = 0; i < in.nseq; ++i)
        if (in.group_of[i] >= g0 && in.group_of[i] < g1) b.add(in, i, in.group_of[i] - g0);
    return b;
}
// A fast form that is abandoned part-way (a later batch or wave overflows) has already counted its earlier
// batches: the statistics of an attempt are kept only when the attempt succeeds — its retries and order
// fallbacks stay counted.
struct StatCheckpoint {
    kh_ctx* c;
    Stats at = c->stat;
    void rollback() const {
        const u64 retries = c->stat.retries, order_fallbacks = c->stat.order_fallbacks;
        c->stat = at;
        c->stat.retries = retries;
        c->stat.order_fallbacks = order_fallbacks;
    }
};
// exp1_fused, and once more with the finer slots an overflowing union asked for; cp: failed attempts are rolled back
static int exp1_fused_rescaled(kh_ctx* c, const Exp1In& in, SubBatch& b, u32 cs, uint64_t* within_hist, uint64_t* across_hist,
                               kh_set** across_set, u32 nwaves, u32 fan_hint, const StatCheckpoint* cp, bool* done) {
    double scale = 0.0;
    KHCHK(exp1_fused(c, b.n(), b.seqs.data(), b.lens.data(), in.on_device, b.group.data(), b.ngroups, in.k, cs, within_hist,
                     across_hist, in.hist_len, b.dist.data(), across_set, done, nwaves, 1.0, &scale, fan_hint));
    if (*done) return KH_OK;
    if (cp) cp->rollback();
    if (scale > 1.0 && scale < 16.0) {
        KHCHK(exp1_fused(c, b.n(), b.seqs.data(), b.lens.data(), in.on_device, b.group.data(), b.ngroups, in.k, cs, within_hist,
                         across_hist, in.hist_len, b.dist.data(), across_set, done, nwaves, scale, nullptr, fan_hint));
        if (!*done && cp) cp->rollback();
    }
    return KH_OK;
}
// One group of more than 64 genomes (exp_type_1.smk:36-61 lists whatever data/dataset_N holds): sub-batches of
// up to 64 genomes, each a fused build + tagged union in which every genome is a group of its own, so that the
// set a sub-batch emits carries "in how many of its genomes"; one counter-summing union of those sets is the
// group's step_3 database (its histogram fused: step_4).
static int exp1_big_group(kh_ctx* c, const Exp1In& in, int g, u64 budget, uint64_t* whist, uint64_t* dist_out /* [nseq] or null */,
                          kh_set** group_set, bool* done) {
    *done = false;
    SubBatch all = groups_batch(in, g, g + 1);
    if (!group_set && whist) {   // histogram and distinct counts only: the super-k-mer form in phases
        const StatCheckpoint cp{c};
        KHCHK(exp1_big_group_skm(c, all.n(), all.seqs.data(), all.lens.data(), in.on_device, in.k, in.cs, whist, in.hist_len,
                                 all.dist.data(), done));
        if (*done) {
            all.scatter(dist_out);
            return KH_OK;
        }
        cp.rollback();
    }
    SetBag subs;
    for (size_t i0 = 0; i0 < all.idx.size(); i0 += KH_TAG_MAX_OPS) {
        const size_t m = std::min<size_t>(KH_TAG_MAX_OPS, all.idx.size() - i0);
        SubBatch b;   // every genome a group of its own
        for (size_t j = i0; j < i0 + m; ++j) b.add(in, all.idx[j], b.ngroups++);
        kh_set* aset = nullptr;
        bool d = false;
        // (a first attempt that overflows in a later wave has counted its earlier waves: rolled back like a single batch's)
        const StatCheckpoint cp{c};
        KHCHK(exp1_fused_rescaled(c, in, b, 0x7fffffffu, nullptr, nullptr, &aset, exp1_waves(b.bases, budget), (u32)m, &cp, &d));
        if (!d) return KH_OK;
        subs.v.push_back(aset);
        b.scatter(dist_out);
    }
    if (group_set) KHCHK(kh_union_sum(c, subs.v.data(), (int)subs.v.size(), in.cs, group_set, whist, whist ? in.hist_len : 0));
    else if (whist) KHCHK(kh_union_histogram(c, subs.v.data(), (int)subs.v.size(), in.cs, whist, in.hist_len));
    *done = true;
    return KH_OK;
}
// Batches of whole groups for the fused forms: a batch holds at most 64 genomes — the width of the genome mask; a
// group of more than 64 genomes is a batch of its own (big, exp1_big_group).  false: a group without genomes.
struct Exp1Batch { int g0, g1; bool big; };
static bool exp1_batches(const Exp1In& in, u64 budget, std::vector<Exp1Batch>* batches) {
    std::vector<u64> gbases(in.ngroups, 0);
    std::vector<int> gcount(in.ngroups, 0);
    for (int i = 0; i < in.nseq; ++i) { gbases[in.group_of[i]] += in.lens[i]; gcount[in.group_of[i]]++; }
    u64 acc_b = 0;
    int acc_n = 0, acc_g = 0, acc_bins = 0, g0 = 0;
    auto close = [&](int g1, bool big) {
        batches->push_back(Exp1Batch{g0, g1, big});
        g0 = g1;
        acc_b = 0; acc_n = acc_g = acc_bins = 0;
    };
    for (int g = 0; g < in.ngroups; ++g) {
        if (gcount[g] == 0) return false;
        if (gcount[g] > KH_TAG_MAX_OPS) {   // wider than the genome mask: a batch of its own, taken in sub-batches
            if (acc_n) close(g, false);
            close(g + 1, true);
            continue;
        }
        // (a batch above the memory budget is run as key-range waves, see exp1_waves: groups are
        // only split into batches by the width of the genome mask)
        const bool fits = acc_n + gcount[g] <= KH_TAG_MAX_OPS && acc_g + 1 <= KH_TAG_MAX_OPS &&
                          acc_bins + gcount[g] + 1 + (acc_g + 2) <= KH_TAG_MAX_BINS &&
                          (acc_b + gbases[g] <= budget || acc_n == 0);
        if (!fits) close(g, false);
        acc_b += gbases[g]; acc_n += gcount[g]; acc_g += 1; acc_bins += gcount[g] + 1;
    }
    if (acc_n || batches->empty()) close(in.ngroups, false);
    return true;
}
// Histograms only, more than 64 genomes: every batch in the super-k-mer form for the within-group
// questions, then ONE more pass over all genomes whose records carry the group number for the
// across-group one.  Anything it cannot take (a region overflow, k outside its range) -> the key arrays.
static int exp1_two_pass(kh_ctx* c, const Exp1In& in, const std::vector<Exp1Batch>& batches, u64 budget, uint64_t* within_hist,
                         uint64_t* across_hist, uint64_t* distinct_per_seq, bool* done) {
    const StatCheckpoint cp{c};
    std::vector<uint64_t> wtmp(within_hist ? (size_t)in.ngroups * in.hist_len : 0), dtmp(in.nseq, 0), atmp(in.hist_len, 0);
    bool ok = true;
    for (const Exp1Batch& bt : batches) {
        uint64_t* wh = within_hist ? wtmp.data() + (size_t)bt.g0 * in.hist_len : nullptr;
        if (bt.big) {
            KHCHK(exp1_big_group(c, in, bt.g0, budget, wh, dtmp.data(), nullptr, &ok));
        } else {
            SubBatch b = groups_batch(in, bt.g0, bt.g1);
            KHCHK(exp1_skm(c, b.view(in), wh, nullptr, b.dist.data(), &ok));
            if (ok) b.scatter(dtmp.data());
        }
        if (!ok) break;
    }
    if (ok) KHCHK(exp1_skm(c, in, nullptr, atmp.data(), nullptr, &ok, /*by_group=*/true));
    if (!ok) {
        cp.rollback();
        return KH_OK;
    }
    if (within_hist) memcpy(within_hist, wtmp.data(), 8 * wtmp.size());
    memcpy(across_hist, atmp.data(), 8 * (size_t)in.hist_len);
    if (distinct_per_seq) memcpy(distinct_per_seq, dtmp.data(), 8 * (size_t)in.nseq);
    *done = true;
    return KH_OK;
}
// Several batches, each in a fused form, and the union of their across-group sets (see kh_exp1_run)
static int exp1_batched(kh_ctx* c, const Exp1In& in, const std::vector<Exp1Batch>& batches, u64 budget, uint64_t* within_hist,
                        uint64_t* across_hist, uint64_t* distinct_per_seq, kh_set** across_set, bool* done) {
    const StatCheckpoint cp{c};
    const bool want_across = across_hist || across_set;
    SetBag asets;
    for (const Exp1Batch& bt : batches) {
        uint64_t* wh = within_hist ? within_hist + (size_t)bt.g0 * in.hist_len : nullptr;
        bool d = false;
        if (bt.big) {   // its across-group set: the group's k-mers, each counted once
            kh_set* gs = nullptr;
            KHCHK(exp1_big_group(c, in, bt.g0, budget, wh, distinct_per_seq, want_across ? &gs : nullptr, &d));
            if (d && gs) {
                kh_set* one = nullptr;
                const int r = kh_set_counts(c, gs, 1, &one);
                kh_set_free(gs);
                KHCHK(r);
                asets.v.push_back(one);
            }
        } else {
            SubBatch b = groups_batch(in, bt.g0, bt.g1);
            kh_set* aset = nullptr;
            if (!want_across)   // steps 1-4 only (more than 64 genomes, no across-group step): the batches are independent
                KHCHK(exp1_skm(c, b.view(in), wh, nullptr, b.dist.data(), &d));
            if (!d)
                KHCHK(exp1_fused(c, b.n(), b.seqs.data(), b.lens.data(), in.on_device, b.group.data(), b.ngroups, in.k, in.cs, wh,
                                 nullptr, in.hist_len, b.dist.data(), want_across ? &aset : nullptr, &d, exp1_waves(b.bases, budget)));
            if (d) {
                if (aset) asets.v.push_back(aset);
                b.scatter(distinct_per_seq);
            }
        }
        if (!d) {
            cp.rollback();
            return KH_OK;
        }
    }
    *done = true;
    if (across_set) return kh_union_sum(c, asets.v.data(), (int)asets.v.size(), in.cs, across_set, across_hist, in.hist_len);
    if (across_hist) return kh_union_histogram(c, asets.v.data(), (int)asets.v.size(), in.cs, across_hist, in.hist_len);
    return KH_OK;
}
// The general path: per-genome sets, per-group unions (steps 1-6), then steps 7+8 over the group sets.
static int exp1_general(kh_ctx* c, const Exp1In& in, uint64_t* within_hist, uint64_t* across_hist, uint64_t* distinct_per_seq,
                        kh_set** group_sets, kh_set** across_set) {
    const int nseq = in.nseq, ngroups = in.ngroups, k = in.k;
    const u32 cs = in.cs, hist_len = in.hist_len;
    SetBag usets, unions, gsets;   // every intermediate set, freed on every way out
    gsets.v.assign(nseq, nullptr);
    unions.v.assign(ngroups, nullptr);
    usets.v.assign(ngroups, nullptr);
    // Groups are independent until step 7, so they are processed in waves that fit a device
    // memory budget (all groups at once for the benchmark sizes; wave by wave for inputs whose
    // k-mers would not fit HBM together): per wave, steps 1+2 build every genome of the wave as
    // a plain set in ONE batched launch sequence, steps 3+4+6 enqueue the wave's group unions
    // back to back before the host waits once; the genome sets are released before the next wave.
    const u64 budget = exp1_wave_bases(c, k);
    std::vector<u64> group_bases(ngroups, 0);
    for (int i = 0; i < nseq; ++i) group_bases[in.group_of[i]] += in.lens[i];
    int r = KH_OK;
    const double t_begin = g_trace ? now_ms() : 0;
    double t_unions_submitted = 0, t_unions_synced = 0, t_groups_done = 0;
    for (int g0 = 0; g0 < ngroups;) {
        if (group_bases[g0] > budget) {             // one group larger than a wave: sub-waves of genomes
            r = group_union_incremental(c, groups_batch(in, g0, g0 + 1).idx, in.seqs, in.lens, in.on_device, k, cs, budget,
                                        within_hist ? within_hist + (size_t)g0 * hist_len : nullptr, hist_len,
                                        distinct_per_seq, &unions.v[g0]);
            if (r == KH_OK) r = kh_set_counts(c, unions.v[g0], 1, &usets.v[g0]);
            if (r != KH_OK) return r;
            ++g0;
            continue;
        }
        int g1 = g0;
        u64 acc = 0;
        while (g1 < ngroups && acc + group_bases[g1] <= budget) acc += group_bases[g1++];
        const SubBatch b = groups_batch(in, g0, g1);
        const std::vector<int>& idx = b.idx;
        std::vector<kh_set*> wsets(idx.size(), nullptr);
        KHCHK(kh_build_batch(c, b.n(), b.seqs.data(), b.lens.data(), in.on_device, k, 1, KH_NO_MAX,
                             KH_KMC_DEFAULT_CS, 0, wsets.data()));
        for (size_t j = 0; j < idx.size(); ++j) {
            gsets.v[idx[j]] = wsets[j];
            if (distinct_per_seq) distinct_per_seq[idx[j]] = wsets[j]->n;
        }
        std::vector<SetopJob> jobs(g1 - g0);
        for (int g = g0; g < g1; ++g) {
            SetopJob& j = jobs[g - g0];
            j.c = c; j.op = KH_OP_UNION; j.mode = KH_OC_SUM; j.cs = cs;
            j.hist = within_hist ? within_hist + (size_t)g * hist_len : nullptr;
            j.hist_len = hist_len;
            for (int i : idx)
                if (in.group_of[i] == g) j.in.push_back(gsets.v[i]);
            if (j.in.empty()) return kh_fail(KH_E_ARG, "group %d has no sequences", g);
            if ((int)j.in.size() > KH_MAX_INPUT_SETS) {   // beyond one launch's fan-in: the general path
                KHCHK(kh_union_sum(c, j.in.data(), (int)j.in.size(), cs, &unions.v[g], j.hist, hist_len));
                j.in.clear();
                continue;
            }
            r = setop_prepare(j);
            if (r == KH_OK) r = setop_plan(j);
            if (r != KH_OK) return r;
        }
        // the slot bounds of all unions of the wave in one launch, then the unions back to back
        Tmp d_bjobs;
        Pinned bpin{c};
        r = setop_bounds_batch(c, jobs, d_bjobs, bpin);
        if (r == KH_OK) {
            std::vector<SetopJob*> run;
            for (auto& j : jobs) run.push_back(&j);
            r = setop_run_batch(c, run.data(), run.size());
        }
        if (r != KH_OK) return r;
        if (g_trace) t_unions_submitted = now_ms();
        if (hipStreamSynchronize(c->st) != hipSuccess) return kh_fail(KH_E_HIP, "stream sync failed");
        if (g_trace) t_unions_synced = now_ms();
        for (int g = g0; g < g1; ++g) {
            if (!jobs[g - g0].in.empty()) KHCHK(setop_finish(jobs[g - g0], &unions.v[g]));
        }
        jobs.clear();
        for (int g = g0; g < g1; ++g) KHCHK(kh_set_counts(c, unions.v[g], 1, &usets.v[g]));
        for (int i : idx) { kh_set_free(gsets.v[i]); gsets.v[i] = nullptr; }   // genome sets of this wave
        g0 = g1;
    }
    // steps 7+8 (skipped when the caller wants neither output: the multi-GPU path does them
    // after exchanging the group sets, khoice_amd/dist.py)
    if (g_trace) t_groups_done = now_ms();
    if (across_set) KHCHK(kh_union_sum(c, usets.v.data(), ngroups, cs, across_set, across_hist, hist_len));   // (nothing fails after it)
    else if (across_hist) KHCHK(kh_union_histogram(c, usets.v.data(), ngroups, cs, across_hist, hist_len));
    if (g_trace)
        fprintf(stderr, "[khoice trace] build submit %.3f wait %.3f | unions submit %.3f wait %.3f finish %.3f | "
                        "across %.3f | total %.3f ms\n",
                g_t_build_submitted - t_begin, g_t_build_synced - g_t_build_submitted,
                t_unions_submitted - g_t_build_synced, t_unions_synced - t_unions_submitted,
                t_groups_done - t_unions_synced, now_ms() - t_groups_done, now_ms() - t_begin);
    if (group_sets)
        for (int g = 0; g < ngroups; ++g) { group_sets[g] = unions.v[g]; unions.v[g] = nullptr; }
    return KH_OK;
}
extern "C" int kh_exp1_run(kh_ctx* c, int nseq, const uint8_t* const* seqs, const uint64_t* lens,
                           int on_device, const int* group_of, int ngroups, int k, uint32_t cs,
                           uint64_t* within_hist, uint64_t* across_hist, uint32_t hist_len,
                           uint64_t* distinct_per_seq, kh_set** group_sets, kh_set** across_set) {
    if (!c || !seqs || !lens || !group_of || nseq <= 0 || ngroups <= 0)
        return kh_fail(KH_E_ARG, "kh_exp1_run: bad argument");
    if ((within_hist || across_hist) && hist_len < 2) return kh_fail(KH_E_ARG, "hist_len must be >= 2");
    for (int i = 0; i < nseq; ++i)
        if (group_of[i] < 0 || group_of[i] >= ngroups)
            return kh_fail(KH_E_ARG, "group_of[%d]=%d outside [0,%d)", i, group_of[i], ngroups);
    KHCHK(check_k(k));
    if (cs < 1) return kh_fail(KH_E_ARG, "cs must be >= 1");
    const Exp1In in{nseq, seqs, lens, on_device, group_of, ngroups, k, cs, hist_len};
    // No per-group database wanted: the fused form (one build in grid mode + one tagged union per
    // BATCH of whole groups; a batch holds at most 64 genomes — the width of the genome mask — and
    // fits the memory budget).  One batch: its histograms are the answer.  Several: each batch also
    // emits its across-group set (counter = groups of the batch holding the k-mer) and one
    // counter-summing union of those sets gives step 7/8.  Anything the fused form cannot take
    // (a group of more than 64 genomes, a slot overflow) falls through to the general path.
    if (!group_sets && !getenv("KHOICE_NO_FUSED")) {
        HIPCHK(hipSetDevice(c->dev));
        const u64 budget = exp1_wave_bases(c, k);
        std::vector<Exp1Batch> batches;
        bool done = false;
        // small k, histograms and distinct counts only: the presence-bitmap form, which has no genome mask and so is
        // tried before the input is cut into batches of 64 genomes
        if (!across_set) KHCHK(exp1_bmp(c, in, within_hist, across_hist, distinct_per_seq, &done));
        if (!done && exp1_batches(in, budget, &batches)) {
            if (batches.size() == 1 && !batches[0].big) {   // all groups in one batch
                const StatCheckpoint cp{c};
                if (!across_set) {   // histograms and distinct counts only: the super-k-mer form
                    KHCHK(exp1_skm(c, in, within_hist, across_hist, distinct_per_seq, &done));
                    if (!done) cp.rollback();
                }
                if (!done) {   // the key arrays, with one more try with finer slots before the general path
                    SubBatch b = groups_batch(in, 0, ngroups);
                    KHCHK(exp1_fused_rescaled(c, in, b, cs, within_hist, across_hist, across_set, exp1_waves(b.bases, budget), 0, &cp, &done));
                    if (done) b.scatter(distinct_per_seq);
                }
            } else {
                if (!across_set && across_hist && ngroups <= KH_TAG_MAX_OPS && !getenv("KHOICE_NO_SKM_TWO_PASS"))
                    KHCHK(exp1_two_pass(c, in, batches, budget, within_hist, across_hist, distinct_per_seq, &done));
                if (!done) KHCHK(exp1_batched(c, in, batches, budget, within_hist, across_hist, distinct_per_seq, across_set, &done));
            }
        }
        if (done) return KH_OK;
    }
    return exp1_general(c, in, within_hist, across_hist, distinct_per_seq, group_sets, across_set);
}

// ------------------------------------------------------------------------------ fused experiment type 2
struct Exp2In {   // the arguments of kh_exp2_run that both forms read
    int nseq; const uint8_t* const* seqs; const uint64_t* lens; int on_device;
    const int* group_of; int ngroups;
    int npivots; const uint8_t* const* pivot_seqs; const uint64_t* pivot_lens; const int* pivot_group;
    int k; u32 cs, hist_len;
};
struct Exp2Out {   // any of them may be NULL
    uint64_t *within_hist, *across_hist, *within_only, *across_only, *distinct_per_seq, *distinct_per_pivot;
    // occ[v] k-mers of pivot p occur in v genomes of its group (across == false) / in v other groups: what
    // `intersect -ocsum` with the -cs{cs} union, then `transform histogram`, and `kmers_subtract` make of them
    void add(const Exp2In& in, int p, bool across, u32 v, u64 occ) const {
        uint64_t* hist = across ? across_hist : within_hist;
        uint64_t* only = across ? across_only : within_only;
        if (v == 0) {
            if (only) only[p] += occ;
        } else if (hist) {
            hist[(size_t)p * in.hist_len + ocsum_bin(v, in.cs, in.hist_len)] += occ;
        }
    }
    void clear(const Exp2In& in) const {
        for (uint64_t* h : {within_hist, across_hist})
            if (h) memset(h, 0, 8 * (size_t)in.npivots * in.hist_len);
        for (uint64_t* o : {within_only, across_only, distinct_per_pivot})
            if (o) memset(o, 0, 8 * (size_t)in.npivots);
        if (distinct_per_seq) memset(distinct_per_seq, 0, 8 * (size_t)in.nseq);
    }
};
// The presence-bitmap form (kh_bmp.hip): the pivots are further operands of the unchanged k_bmp_build, k_bmp_pivot
// counts every pivot's word against the bit-sliced counter of its group and against the counter over groups.  *done ==
// false: the form does not apply (nothing was launched, no retry is counted).
static int exp2_bmp(kh_ctx* c, const Exp2In& in, const Exp2Out& out, bool* done) {
    *done = false;
    const int k = in.k, nseq = in.nseq, ngroups = in.ngroups, npiv = in.npivots, nops = nseq + npiv;
    if (!bmp_form_k(k) || (u32)ngroups > KH_BMP_MAX_COUNT) return KH_OK;
    // ---- operands in group-major order: the genomes of a group, then its pivots
    const BmpOperands o = bmp_operands(nseq, in.seqs, in.lens, in.group_of, ngroups, npiv, in.pivot_seqs, in.pivot_lens, in.pivot_group);
    std::vector<KhBmpPivotGroup> groups(ngroups, KhBmpPivotGroup{0, 0, 0, 0, 0, 0});
    for (int p = 0; p < npiv; ++p) groups[in.pivot_group[p]].npiv++;
    u32 prows = 0, q0 = 0;
    u64 nbins = 0;
    for (int g = 0; g < ngroups; ++g) {
        KhBmpPivotGroup& gr = groups[g];
        if (o.size[g] > KH_BMP_MAX_COUNT) return KH_OK;
        gr.first = o.first[g];
        gr.size = o.size[g];
        gr.q0 = q0;
        if (gr.npiv) gr.prow = prows++;
        q0 += gr.npiv;
        nbins += (u64)gr.npiv * (gr.size + 1 + (u32)ngroups);
    }
    if (nbins + (u64)nops > KH_BMP_MAX_BINS) return KH_OK;
    std::vector<int> q_of_pivot(npiv);   // pivots in group-major order, with their bins
    std::vector<KhBmpPivot> pivots(npiv);
    {
        std::vector<u32> qat(ngroups);
        for (int g = 0; g < ngroups; ++g) qat[g] = groups[g].q0;
        for (int p = 0; p < npiv; ++p) {
            const int g = in.pivot_group[p];
            q_of_pivot[p] = (int)qat[g]++;
            pivots[q_of_pivot[p]] = KhBmpPivot{(u32)o.op_of_pivot[p], (u32)g, 0, 0};
        }
        u32 b = 0;
        for (KhBmpPivot& pv : pivots) {
            pv.bin0 = b;
            pv.abin0 = b + groups[pv.group].size + 1;
            b = pv.abin0 + (u32)ngroups;
        }
    }
    BmpRun run(c, k, in.on_device, o);
    bool fits = false;
    KHCHK(run.plan(prows, &fits));
    if (!fits) return KH_OK;
    run.layout(1, (u32)nbins + (u32)nops);
    const size_t off_groups = run.table(groups), off_pivots = run.table(pivots);
    Tmp d_present;
    TMP_ALLOC(d_present, c, (size_t)(std::max<u64>(1, prows) * run.s.nwords * 8));
    KHCHK(run.upload());
    KHCHK(run.build());
    KhBmpPivotJob job;
    job.ops = run.ops();
    job.groups = run.dev<const KhBmpPivotGroup>(off_groups);
    job.pivots = run.dev<const KhBmpPivot>(off_pivots);
    job.partial = run.d_partial.as<u64>();
    job.present = d_present.as<u64>();
    job.hist = run.hist(0);
    job.nwords = run.s.nwords;
    job.nops = (u32)nops; job.ngroups = (u32)ngroups; job.npivots = (u32)npiv; job.nbins = (u32)nbins; job.reps = run.reps;
    KHCHK(timed_launch(c, KC_BMP_PIVOT, [&] { kh_launch_bmp_pivot(job, run.s.rgrid, run.s.rwaves, c->st); }));
    KHCHK(run.download());

    // ---- the bins folded
    std::vector<u64> bins;
    run.bins(0, run.nb, &bins);
    out.clear(in);
    const u64 dsum = run.distinct(bins, nbins, out.distinct_per_seq);
    u64 held = 0;
    for (int p = 0; p < npiv; ++p) {
        const KhBmpPivot& pv = pivots[q_of_pivot[p]];
        if (out.distinct_per_pivot) out.distinct_per_pivot[p] = bins[nbins + pv.op];
        for (u32 v = 0; v <= groups[pv.group].size; ++v) out.add(in, p, false, v, bins[pv.bin0 + v]);
        for (u32 v = 0; v < (u32)ngroups; ++v) out.add(in, p, true, v, bins[pv.abin0 + v]);
        held += bins[nbins + pv.op] - bins[pv.bin0];
    }
    run.account(dsum, held);   // pivot k-mers their own group holds
    *done = true;
    return KH_OK;
}
// The super-k-mer form (k_skm_cross with the read-out SkmCrossOwn, kh_skm_device.h; k = 17 .. 63, taken only with KHOICE_EXP2_SKM=1 — the set form
// stays the default): exp3_skm's run with the type-2 read-out on the slot walk.  Genomes and pivots go through the
// unchanged scatter and regroup as ONE list of texts, the pivots behind the genomes and every pivot a group of its own
// to TagLayout (its tag is nseq + q); the kernel learns a pivot's OWN group from KhSkmPivotJob::pinfo.  A pass takes
// pivots in the caller's order while genomes + pivots <= 64 and their bins (size of the own group + 1 within, ngroups
// across) <= 1024; every pass stages, scatters and walks the genomes AGAIN (exp3_skm's known waste), the genomes'
// distinct counts are the first pass's.  *done == false and no retry counted: the form does not apply (switch, k,
// KHOICE_NO_SKM / KHOICE_NO_SKM2, no pivot, more than 63 genomes, a pass without a k-mer position, geometry, memory),
// nothing of the outputs was written.  A capacity or order error of a kernel, more spilled records or listed slots than
// are kept, or a later pass that does not stage: retries++, and the set form answers.
static int exp2_skm(kh_ctx* c, const Exp2In& in, const Exp2Out& out, bool* done) {
    *done = false;
    const int k = in.k, nseq = in.nseq, ngroups = in.ngroups, npiv = in.npivots;
    const char* sw = getenv("KHOICE_EXP2_SKM");
    if (!sw || atoi(sw) != 1 || !skm_form_k(k)) return KH_OK;
    if (!npiv || nseq >= KH_TAG_MAX_OPS) return KH_OK;
    constexpr u32 max_bins = 1024;   // SKM_CROSS_BINS of kh_skm_device.h: the bins the walk keeps in LDS
    std::vector<u32> gsize(ngroups, 0), gstart(ngroups, 0);   // group-major order, as TagLayout numbers the operands
    u32 fan = 1;
    for (int i = 0; i < nseq; ++i) fan = std::max(fan, ++gsize[in.group_of[i]]);
    for (int g = 1; g < ngroups; ++g) gstart[g] = gstart[g - 1] + gsize[g - 1];
    auto bins_of = [&](int p) { return gsize[in.pivot_group[p]] + 1 + (u32)ngroups; };
    std::vector<int> pass0;   // first pivot of every pass, and npiv
    {
        u32 bins = 0;
        for (int p = 0; p < npiv; ++p) {
            const int np = pass0.empty() ? 0 : p - pass0.back();
            if (pass0.empty() || nseq + np + 1 > KH_TAG_MAX_OPS || bins + bins_of(p) > max_bins) {
                pass0.push_back(p);
                bins = 0;
            }
            bins += bins_of(p);
        }
        pass0.push_back(npiv);
    }
    const int npasses = (int)pass0.size() - 1;
    u64 gbases = 0, pbases = 0;
    const u64 gpos = kmer_positions(nseq, in.lens, k, &gbases);
    for (int b = 0; b < npasses; ++b)   // (a pass without a k-mer position has no geometry)
        if (!(gpos + kmer_positions(pass0[b + 1] - pass0[b], in.pivot_lens + pass0[b], k))) return KH_OK;
    kmer_positions(npiv, in.pivot_lens, k, &pbases);
    const KhSkmWidth& wd = kh_skm_width(k > KH_SKM_MAX_K);
    std::vector<u64> dseq(nseq, 0), dpiv(npiv, 0);
    std::vector<std::vector<u64>> occ(npiv);   // occ[p]: the pivot's within bins, then its across bins
    u64 kmers = 0, records = 0, multi = 0, big = 0;
    for (int b = 0; b < npasses; ++b) {
        const int p0 = pass0[b], np = pass0[b + 1] - p0, nops = nseq + np;
        std::vector<const uint8_t*> seqs(in.seqs, in.seqs + nseq);
        std::vector<uint64_t> lens(in.lens, in.lens + nseq);
        std::vector<int> group_of(in.group_of, in.group_of + nseq);
        KhSkmPivotJob pj{};
        KhSkmCrossJob& cj = pj.cj;
        for (int q = 0; q < np; ++q) {
            seqs.push_back(in.pivot_seqs[p0 + q]);
            lens.push_back(in.pivot_lens[p0 + q]);
            group_of.push_back(ngroups + q);
            const int g = in.pivot_group[p0 + q];
            pj.pinfo[nseq + q] = gstart[g] | (gsize[g] << 8) | (cj.nbins << 16);
            cj.nbins += bins_of(p0 + q);
        }
        SkmRun s(c);
        // fan hint: a pivot brings its copy of a locus to the slot of the group it was held out of — one more than the
        // largest group
        KHCHK(skm_prepare(c, nops, seqs.data(), lens.data(), in.on_device, group_of.data(), ngroups + np, k, false, 0, fan + 1, &s, wd.cross_round));
        if (!s.staged) {
            if (b) c->stat.retries++;   // (a later pass whose geometry or memory does not fit: work was done for nothing)
            return KH_OK;
        }
        const KhSkmJob& job = s.job;
        hipStream_t st = c->st;
        cj.ngenomes = (u32)nseq;
        const u64 pm = ((1ull << np) - 1ull) << nseq;   // (1 <= np <= 63)
        cj.pmlo = (u32)pm; cj.pmhi = (u32)(pm >> 32);
        const u32 grid = std::min<u32>(s.g.nslots, wd.pivot_per_cu * (u32)std::max(1, c->cus));
        cj.reps = std::min<u32>(grid, 64);
        const size_t bins_bytes = 8 * (size_t)cj.reps * cj.nbins;
        Tmp d_bins;
        TMP_ALLOC(d_bins, c, bins_bytes);
        Pinned pin{c};
        PIN_ALLOC(pin, bins_bytes);
        cj.bins = d_bins.as<unsigned long long>();
        HIPCHK(hipMemsetAsync(cj.bins, 0, bins_bytes, st));
        KHCHK(timed_launch(c, KC_SKM_CROSS, [&] { wd.pivot(job, pj, grid, st); }));
        bool declines = false;
        KHCHK(s.settle(s.off.ctl, [&](u32 nlisted) {   // ([ctl .. dup] of the workspace; the bins are read back below)
            big += nlisted;
            cj.nlisted = nlisted;
            return timed_launch(c, KC_SKM_CROSS, [&] { wd.pivot(job, pj, nlisted, st); });
        }, &declines));
        if (declines) return KH_OK;   // the set form takes over
        HIPCHK(hipMemcpyAsync(pin.p, cj.bins, bins_bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        records += s.h_ctl()[KH_SKM_CTL_RECORDS];
        multi += s.h_ctl()[KH_SKM_CTL_MULTI];
        s.per_text([&](int t, u64 inst, u64 d) {   // text t of this pass: the genomes, then its pivots
            if (t >= nseq) { dpiv[p0 + t - nseq] = d; kmers += inst; }
            else if (b == 0) { dseq[t] = d; kmers += inst; }
        });
        const u64* h_bins = static_cast<const u64*>(pin.p);
        for (int q = 0; q < np; ++q) {
            const u32 w0 = pj.pinfo[nseq + q] >> 16, n = bins_of(p0 + q);
            std::vector<u64>& o = occ[p0 + q];
            o.assign(n, 0);
            for (u32 r = 0; r < cj.reps; ++r)
                for (u32 i = 0; i < n; ++i) o[i] += h_bins[(size_t)r * cj.nbins + w0 + i];
        }
    }
    // ---- every pass went through.  Every distinct k-mer of a pivot was counted once within and once across
    for (int p = 0; p < npiv; ++p) {
        const u32 nw = gsize[in.pivot_group[p]] + 1;
        u64 ws = 0, as = 0;
        for (u32 i = 0; i < nw; ++i) ws += occ[p][i];
        for (u32 i = 0; i < (u32)ngroups; ++i) as += occ[p][nw + i];
        if (ws != dpiv[p] || as != dpiv[p])
            return kh_fail(KH_E_INTERNAL, "kh_exp2_run: pivot %d has %llu distinct k-mers, its within bins hold %llu and its across bins %llu",
                           p, (unsigned long long)dpiv[p], (unsigned long long)ws, (unsigned long long)as);
    }
    // ---- the outputs, and the accounting of exp2_bmp
    out.clear(in);
    u64 dsum = 0, held = 0;
    for (int i = 0; i < nseq; ++i) {
        dsum += dseq[i];
        if (out.distinct_per_seq) out.distinct_per_seq[i] = dseq[i];
    }
    for (int p = 0; p < npiv; ++p) {
        const u32 nw = gsize[in.pivot_group[p]] + 1;
        dsum += dpiv[p];
        if (out.distinct_per_pivot) out.distinct_per_pivot[p] = dpiv[p];
        for (u32 v = 0; v < nw; ++v) out.add(in, p, false, v, occ[p][v]);
        for (u32 v = 0; v < (u32)ngroups; ++v) out.add(in, p, true, v, occ[p][nw + v]);
        held += dpiv[p] - occ[p][0];
    }
    c->stat.skm_records += records;
    c->stat.cross_multi_slots += multi;
    c->stat.big_slots += big;
    c->stat.bases += gbases + pbases;
    c->stat.builds += (u64)nseq + (u64)npiv;
    c->stat.kmers += kmers;
    c->stat.distinct += dsum;
    c->stat.setop_in += dsum;
    c->stat.setop_out += held;   // pivot k-mers their own group holds
    c->stat.setops++;
    *done = true;
    return KH_OK;
}
// The set form: the calls of exp_type_2.smk:289-507 on sets that stay in device memory — one batched plain build of
// genomes and pivots, the -cs{cs} union of every group, set_counts 1, per pivot group the union of the other groups,
// and intersect -ocsum / kmers_subtract of every pivot with both.
static int exp2_sets(kh_ctx* c, const Exp2In& in, const Exp2Out& out) {
    const int nseq = in.nseq, ngroups = in.ngroups, npiv = in.npivots;
    SetBag plain, unions, gsets, others;   // every intermediate set, freed on every way out
    KHCHK(build_plain(c, nseq, in.seqs, in.lens, npiv, in.pivot_seqs, in.pivot_lens, in.on_device, in.k, &plain));
    out.clear(in);
    for (int i = 0; i < nseq; ++i)
        if (out.distinct_per_seq) out.distinct_per_seq[i] = plain.v[i]->n;
    std::vector<int> has_pivot(ngroups, 0);
    for (int p = 0; p < npiv; ++p) has_pivot[in.pivot_group[p]] = 1;
    KHCHK(group_unions(c, plain.v.data(), nseq, in.group_of, ngroups, in.cs, &unions, nullptr, 0));
    KHCHK(group_ones(c, unions, &gsets));
    others.v.assign(ngroups, nullptr);
    for (int g = 0; g < ngroups && ngroups > 1; ++g) {
        if (!has_pivot[g]) continue;
        std::vector<const kh_set*> rest;
        for (int h = 0; h < ngroups; ++h)
            if (h != g) rest.push_back(gsets.v[h]);
        KHCHK(kh_union_sum(c, rest.data(), (int)rest.size(), in.cs, &others.v[g], nullptr, 0));
    }
    std::vector<uint64_t> hist(in.hist_len);
    for (int p = 0; p < npiv; ++p) {
        const kh_set* pivot = plain.v[nseq + p];
        const int g = in.pivot_group[p];
        if (out.distinct_per_pivot) out.distinct_per_pivot[p] = pivot->n;
        for (int across = 0; across < 2; ++across) {
            const kh_set* other = across ? others.v[g] : unions.v[g];
            uint64_t* h = across ? out.across_hist : out.within_hist;
            uint64_t* only = across ? out.across_only : out.within_only;
            if (!other) {   // one group: nothing to meet, the pivot's k-mers are all its own
                if (only) only[p] = pivot->n;
                continue;
            }
            if (h) {
                SetBag r;
                KHCHK(kh_simple(c, pivot, other, KH_INTERSECT, KH_MODE_SUM, in.cs, r.slot()));
                KHCHK(kh_histogram(c, r.v[0], hist.data(), in.hist_len));
                memcpy(h + (size_t)p * in.hist_len, hist.data(), 8 * (size_t)in.hist_len);
            }
            if (only) {
                SetBag r;
                KHCHK(kh_simple(c, pivot, other, KH_KMERS_SUBTRACT, KH_MODE_LEFT, in.cs, r.slot()));
                only[p] = r.v[0]->n;
            }
        }
    }
    return KH_OK;
}
extern "C" int kh_exp2_run(kh_ctx* c, int nseq, const uint8_t* const* seqs, const uint64_t* lens, int on_device,
                           const int* group_of, int ngroups, int npivots, const uint8_t* const* pivot_seqs,
                           const uint64_t* pivot_lens, const int* pivot_group, int k, uint32_t cs, uint64_t* within_hist,
                           uint64_t* across_hist, uint32_t hist_len, uint64_t* within_only, uint64_t* across_only,
                           uint64_t* distinct_per_seq, uint64_t* distinct_per_pivot) {
    KHCHK(exp_check_args("kh_exp2_run", c, nseq, seqs, lens, group_of, ngroups, npivots, pivot_seqs, pivot_lens, true, pivot_group,
                         hist_len, k, cs, nullptr));
    const Exp2In in{nseq, seqs, lens, on_device, group_of, ngroups, npivots, pivot_seqs, pivot_lens, pivot_group, k, cs, hist_len};
    const Exp2Out out{within_hist, across_hist, within_only, across_only, distinct_per_seq, distinct_per_pivot};
    HIPCHK(hipSetDevice(c->dev));
    bool done = false;
    KHCHK(exp2_bmp(c, in, out, &done));
    if (done) return KH_OK;
    KHCHK(exp2_skm(c, in, out, &done));   // (KHOICE_EXP2_SKM=1 only)
    if (done) return KH_OK;
    return exp2_sets(c, in, out);
}

// ------------------------------------------------------------------------------ fused experiment type 4
struct Exp4In {   // the arguments of kh_exp4_run that both forms read
    int nseq; const uint8_t* const* seqs; const uint64_t* lens; int on_device;
    const int* group_of; int ngroups;
    int npivots; const uint8_t* const* pivot_seqs; const uint64_t* pivot_lens;
    int k; u32 cs, pivot_cs, hist_len;
};
struct Exp4Out {   // any of them may be NULL
    uint64_t* within_hist; double* rows; uint64_t *unique_pivot_count, *distinct_per_seq, *distinct_per_pivot;
    void set_row(const Exp4In& in, int p, const double* row, uint64_t uniq) const {
        if (rows) memcpy(rows + (size_t)p * in.ngroups, row, sizeof(double) * (size_t)in.ngroups);
        if (unique_pivot_count) unique_pivot_count[p] = uniq;
    }
};
// The presence-bitmap form (kh_bmp.hip): genomes (group-major) and pivots are the operands of the unchanged
// k_bmp_build; k_bmp_count adds up the pivots' multiplicities, k_bmp_present leaves the within-group bins, the groups'
// presence words and the pivots' words, k_bmp_member writes every pivot's (mask, count) records in code order, which is
// the `dump -s` order: the host only copies them and sums.  *done == false: the form does not apply (nothing was
// launched, no retry is counted).
static int exp4_bmp(kh_ctx* c, const Exp4In& in, const Exp4Out& out, bool* done) {
    *done = false;
    const int k = in.k, nseq = in.nseq, ngroups = in.ngroups, npiv = in.npivots, nops = nseq + npiv;
    if (!bmp_form_k(k) || (u32)ngroups > KH_BMP_MEMBER_GROUPS) return KH_OK;
    // ---- operands: the genomes in group-major order, then the pivots
    const BmpOperands o = bmp_operands(nseq, in.seqs, in.lens, in.group_of, ngroups, npiv, in.pivot_seqs, in.pivot_lens);
    std::vector<KhBmpGroup> groups;
    u64 nbins = 0;
    if (!bmp_group_table(o, &groups, &nbins)) return KH_OK;
    if (nbins + (u64)nops > KH_BMP_MAX_BINS) return KH_OK;
    // ---- memory beside the partial bitmaps, in rows of one bitmap: present, pword, the count tables (32 rows each:
    // 4^k cells of 4 bytes) and the records (12 bytes each, at most one per position and per code of a pivot)
    const u64 nwords = k >= 3 ? 1ull << (2 * k - 6) : 1, ncells = 64 * nwords, ncodes = 1ull << (2 * k);
    std::vector<u64> rec_off(std::max(1, npiv), 0);
    u64 nrec_max = 0;
    for (int p = 0; p < npiv; ++p) {
        const u64 npos = in.pivot_lens[p] >= (u64)k ? in.pivot_lens[p] - k + 1 : 0;
        if (npos >> 32) return KH_OK;   // (the cells of the count table are 32 bits wide)
        rec_off[p] = nrec_max;
        nrec_max += std::min(npos, ncodes);
    }
    const u64 extra_rows = (u64)ngroups + 33ull * (u64)npiv + (12 * nrec_max + 8 * nwords - 1) / (8 * nwords);
    BmpRun run(c, k, in.on_device, o);
    bool fits = false;
    KHCHK(run.plan(extra_rows, &fits));
    if (!fits) return KH_OK;

    hipStream_t st = c->st;
    const u32 nblocks = (u32)((nwords + 63) / 64);
    run.layout(1, (u32)nbins + (u32)nops);
    const size_t off_groups = run.table(groups), off_rec = run.table(rec_off);
    Tmp d_present, d_pword, d_cnt, d_blk, d_rmask, d_rcount;
    TMP_ALLOC(d_present, c, (size_t)((u64)ngroups * nwords * 8));
    TMP_ALLOC(d_pword, c, (size_t)(std::max<u64>(1, npiv) * nwords * 8));
    TMP_ALLOC(d_cnt, c, (size_t)(std::max<u64>(1, npiv) * ncells * 4));
    TMP_ALLOC(d_blk, c, (size_t)(std::max<u64>(1, npiv) * nblocks * 4));
    TMP_ALLOC(d_rmask, c, (size_t)(std::max<u64>(1, nrec_max) * 8));
    TMP_ALLOC(d_rcount, c, (size_t)(std::max<u64>(1, nrec_max) * 4));
    KHCHK(run.upload([&] {
        if (npiv) HIPCHK(hipMemsetAsync(d_cnt.b->p, 0, (size_t)((u64)npiv * ncells * 4), st));
        return (int)KH_OK;
    }));
    KHCHK(run.build());
    KhBmpMemberJob job{};
    job.splits = run.dev<const KhBmpSplit>(run.off_splits);
    job.ops = run.ops();
    job.groups = run.dev<const KhBmpGroup>(off_groups);
    job.partial = run.d_partial.as<u64>();
    job.present = d_present.as<u64>();
    job.pword = d_pword.as<u64>();
    job.cnt = d_cnt.as<u32>();
    job.blk = d_blk.as<u32>();
    job.hist = run.hist(0);
    job.rec_off = run.dev<const u64>(off_rec);
    job.rec_mask = d_rmask.as<u64>();
    job.rec_count = d_rcount.as<u32>();
    job.nwords = nwords; job.ncells = ncells;
    job.nops = (u32)nops; job.ngenomes = (u32)nseq; job.ngroups = (u32)ngroups; job.npivots = (u32)npiv;
    job.nbins = (u32)nbins; job.reps = run.reps; job.nblocks = nblocks;
    job.psplit0 = npiv ? run.s.ops[nseq].split0 : (u32)run.s.nsplits;
    job.npsplits = (u32)run.s.nsplits - job.psplit0;
    job.tile_pos = run.s.tile_pos; job.pivot_cs = in.pivot_cs; job.k = k;
    if (npiv) KHCHK(timed_launch(c, KC_BMP_COUNT, [&] { kh_launch_bmp_count(job, st); }));
    KHCHK(timed_launch(c, KC_BMP_PRESENT, [&] { kh_launch_bmp_present(job, run.s.rgrid, run.s.rwaves, st); }));
    if (npiv) KHCHK(timed_launch(c, KC_BMP_MEMBER, [&] { kh_launch_bmp_member(job, st); }));
    KHCHK(run.download());

    // ---- the bins folded as exp1_bmp folds them
    std::vector<u64> bins;
    run.bins(0, run.nb, &bins);
    fold_within(groups, bins, in.cs, out.within_hist, in.hist_len);
    const u64 dsum = run.distinct(bins, nbins, out.distinct_per_seq);
    u64 nrec = 0;
    std::vector<u64> h_off(std::max(1, npiv), 0);   // the records in host memory: packed, the exact numbers
    for (int p = 0; p < npiv; ++p) {
        const u64 n = bins[nbins + nseq + p];
        if (out.distinct_per_pivot) out.distinct_per_pivot[p] = n;
        if (n > (p + 1 < npiv ? rec_off[p + 1] : nrec_max) - rec_off[p])
            return kh_fail(KH_E_INTERNAL, "exp4_bmp: pivot %d has %llu records, more than its positions", p, (unsigned long long)n);
        h_off[p] = nrec;
        nrec += n;
    }
    // ---- every pivot's records copied, then summed in order: the pivots are independent, a few host threads share them
    if (npiv && nrec && (out.rows || out.unique_pivot_count)) {
        Pinned rpin{c};
        const size_t off_cnt = (8 * (size_t)nrec + 63) & ~(size_t)63;
        PIN_ALLOC(rpin, off_cnt + 4 * (size_t)nrec + 64);
        u64* h_mask = static_cast<u64*>(rpin.p);
        u32* h_cnt = reinterpret_cast<u32*>(static_cast<u8*>(rpin.p) + off_cnt);
        for (int p = 0; p < npiv; ++p) {
            const u64 n = bins[nbins + nseq + p];
            if (!n) continue;
            HIPCHK(hipMemcpyAsync(h_mask + h_off[p], job.rec_mask + rec_off[p], 8 * (size_t)n, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h_cnt + h_off[p], job.rec_count + rec_off[p], 4 * (size_t)n, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        std::atomic<int> next{0};
        auto work = [&]() {
            std::vector<double> row(ngroups);
            for (int p = next.fetch_add(1); p < npiv; p = next.fetch_add(1)) {
                uint64_t uniq = 0;
                confusion_sum(h_mask + h_off[p], h_cnt + h_off[p], nullptr, bins[nbins + nseq + p], 1, ngroups, row.data(), &uniq);
                out.set_row(in, p, row.data(), uniq);
            }
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < std::min(16, npiv); ++t) pool.emplace_back(work);
        work();
        for (std::thread& t : pool) t.join();
    } else {
        const std::vector<double> zero(ngroups, 0.0);
        for (int p = 0; p < npiv; ++p) out.set_row(in, p, zero.data(), 0);
    }
    run.account(dsum, nrec);   // membership records
    *done = true;
    return KH_OK;
}
// The set form: the calls of workflow/exp_type_4.py::run_batched on sets that stay in device memory — one batched plain
// build of the genomes, one counted build of the pivots, the -cs{cs} union of every group with its histogram,
// set_counts 1, and per pivot the membership search and the sum of kh_confusion_row.
static int exp4_sets(kh_ctx* c, const Exp4In& in, const Exp4Out& out) {
    const int nseq = in.nseq, ngroups = in.ngroups, npiv = in.npivots;
    SetBag plain, pivots, unions, gsets;   // every intermediate set, freed on every way out
    KHCHK(build_plain(c, nseq, in.seqs, in.lens, 0, nullptr, nullptr, in.on_device, in.k, &plain));
    pivots.v.assign(npiv, nullptr);
    if (npiv)
        KHCHK(kh_build_batch(c, npiv, in.pivot_seqs, in.pivot_lens, in.on_device, in.k, 1, KH_NO_MAX, in.pivot_cs, 1, pivots.v.data()));
    for (int i = 0; i < nseq; ++i)
        if (out.distinct_per_seq) out.distinct_per_seq[i] = plain.v[i]->n;
    KHCHK(group_unions(c, plain.v.data(), nseq, in.group_of, ngroups, in.cs, &unions, out.within_hist, in.hist_len));
    KHCHK(group_ones(c, unions, &gsets));
    std::vector<double> row(ngroups);
    for (int p = 0; p < npiv; ++p) {
        const kh_set* pivot = pivots.v[p];
        if (out.distinct_per_pivot) out.distinct_per_pivot[p] = pivot->n;
        if (!out.rows && !out.unique_pivot_count) continue;
        Membership m;
        KHCHK(membership_compute(c, pivot, gsets.v.data(), ngroups, m));
        uint64_t uniq = 0;
        confusion_sum(m.masks.data(), m.counts.data(), m.order.data(), pivot->n, m.nwords, ngroups, row.data(), &uniq);
        out.set_row(in, p, row.data(), uniq);
    }
    return KH_OK;
}
extern "C" int kh_exp4_run(kh_ctx* c, int nseq, const uint8_t* const* seqs, const uint64_t* lens, int on_device,
                           const int* group_of, int ngroups, int npivots, const uint8_t* const* pivot_seqs,
                           const uint64_t* pivot_lens, int k, uint32_t cs, uint32_t pivot_cs, uint64_t* within_hist,
                           uint32_t hist_len, double* rows, uint64_t* unique_pivot_count, uint64_t* distinct_per_seq,
                           uint64_t* distinct_per_pivot) {
    KHCHK(exp_check_args("kh_exp4_run", c, nseq, seqs, lens, group_of, ngroups, npivots, pivot_seqs, pivot_lens, false, nullptr,
                         hist_len, k, cs, &pivot_cs));
    const Exp4In in{nseq, seqs, lens, on_device, group_of, ngroups, npivots, pivot_seqs, pivot_lens, k, cs, pivot_cs, hist_len};
    const Exp4Out out{within_hist, rows, unique_pivot_count, distinct_per_seq, distinct_per_pivot};
    HIPCHK(hipSetDevice(c->dev));
    bool done = false;
    KHCHK(exp4_bmp(c, in, out, &done));
    if (done) return KH_OK;
    return exp4_sets(c, in, out);
}

// ------------------------------------------------------------------------------ fused experiment type 6
// exp_type_6.smk:164-344 has the rules of type 4 up to the last one, which runs src/merge_lists.py with -r: per read the
// votes over the groups' k-mer sets.  No pivot database: every k-mer of a read is in the database built from the same
// reads, so the KeyError of :167 cannot happen and there is nothing to check against.
struct Exp6In {   // the arguments of kh_exp6_run that every form reads
    int nseq; const uint8_t* const* seqs; const uint64_t* lens; int on_device;
    const int* group_of; int ngroups;
    int npivots; const uint8_t* const* pivot_reads; const uint64_t* const* pivot_read_off; const uint64_t* pivot_nreads;
    int k; u32 cs, hist_len;
};
struct Exp6Out {   // within_hist, unmatched and distinct_per_seq may be NULL
    uint64_t* within_hist; uint64_t* tie_masks; uint32_t* unmatched; uint64_t* distinct_per_seq;
};
// The presence-bitmap form (kh_bmp.hip, kh_reads.hip): the genomes (group-major) are the operands of the unchanged
// k_bmp_build; k_bmp_present without pivots leaves the within-group bins, the distinct counters and the groups' presence
// words; k_bmp_group_masks transposes those into the mask table; per pivot the batches of read_votes_batches, whose masks
// k_read_lookup loads from the table by the window's canonical code.  *done == false: the form does not apply (nothing
// was launched, no retry is counted).
static int exp6_bmp(kh_ctx* c, const Exp6In& in, const Exp6Out& out, bool* done) {
    *done = false;
    const int k = in.k, nseq = in.nseq, ngroups = in.ngroups;
    if (!bmp_form_k(k) || (u32)ngroups > KH_READS_MAX_SETS) return KH_OK;   // (too many groups: the set form reports them)
    const BmpOperands o = bmp_operands(nseq, in.seqs, in.lens, in.group_of, ngroups);   // (reads are not operands)
    std::vector<KhBmpGroup> groups;
    u64 nbins = 0;
    if (!bmp_group_table(o, &groups, &nbins)) return KH_OK;
    if (nbins + (u64)nseq > KH_BMP_MAX_BINS) return KH_OK;
    // ---- memory beside the partial bitmaps, in rows of one bitmap: present, and the table (64 nwords cells of mwords
    // words: 64 mwords rows)
    const u64 nwords = k >= 3 ? 1ull << (2 * k - 6) : 1;
    const u32 mwords = (u32)std::max(1, (ngroups + 63) / 64);
    BmpRun run(c, k, in.on_device, o);
    bool fits = false;
    KHCHK(run.plan((u64)ngroups + 64ull * mwords, &fits));
    if (!fits) return KH_OK;

    hipStream_t st = c->st;
    run.layout(1, (u32)nbins + (u32)nseq);
    const size_t off_groups = run.table(groups);
    Tmp d_present, d_table;
    TMP_ALLOC(d_present, c, (size_t)((u64)ngroups * nwords * 8));
    TMP_ALLOC(d_table, c, (size_t)(64 * nwords * mwords * 8));
    KHCHK(run.upload());
    KHCHK(run.build());
    KhBmpMemberJob job{};            // no pivots: pword, cnt, blk and the records stay null and untouched
    job.splits = run.dev<const KhBmpSplit>(run.off_splits);
    job.ops = run.ops();
    job.groups = run.dev<const KhBmpGroup>(off_groups);
    job.partial = run.d_partial.as<u64>();
    job.present = d_present.as<u64>();
    job.hist = run.hist(0);
    job.nwords = nwords; job.ncells = 64 * nwords;
    job.nops = (u32)nseq; job.ngenomes = (u32)nseq; job.ngroups = (u32)ngroups; job.npivots = 0;
    job.nbins = (u32)nbins; job.reps = run.reps; job.nblocks = (u32)((nwords + 63) / 64);
    job.psplit0 = (u32)run.s.nsplits; job.npsplits = 0;
    job.tile_pos = run.s.tile_pos; job.pivot_cs = 1; job.k = k;
    KHCHK(timed_launch(c, KC_BMP_PRESENT, [&] { kh_launch_bmp_present(job, run.s.rgrid, run.s.rwaves, st); }));
    KHCHK(timed_launch(c, KC_BMP_GROUP_MASKS,
                       [&] { kh_launch_bmp_group_masks(d_present.as<u64>(), d_table.as<u64>(), nwords, (u32)ngroups, mwords, st); }));
    KHCHK(run.download());
    run.d_partial.release();         // the votes need the table alone: their mask buffer is sized by what is free now
    d_present.release();

    // ---- the bins folded as exp1_bmp folds them
    std::vector<u64> bins;
    run.bins(0, run.nb, &bins);
    fold_within(groups, bins, in.cs, out.within_hist, in.hist_len);
    u64 in_groups = 0;               // the groups' distinct k-mers: what the unions of the set form put out
    for (const KhBmpGroup& g : groups)
        for (u32 cnt = 1; cnt <= g.size; ++cnt) in_groups += bins[g.bin0 + cnt];
    run.account(run.distinct(bins, nbins, out.distinct_per_seq), in_groups);

    // ---- the votes, pivot by pivot
    const u64* table = d_table.as<u64>();
    u64 r0 = 0;
    for (int p = 0; p < in.npivots; ++p) {
        if (!in.pivot_read_off[p]) return kh_fail(KH_E_ARG, "kh_read_votes: NULL argument");   // (as the set form's call says it)
        KHCHK(read_votes_batches(c, in.pivot_reads[p], in.pivot_read_off[p], in.pivot_nreads[p], in.on_device, k, ngroups,
                                 out.tie_masks ? out.tie_masks + r0 * mwords : nullptr, nullptr, out.unmatched ? out.unmatched + r0 : nullptr,
                                 [&](KhReadsJob& rj) { return timed_launch(c, KC_READ_LOOKUP, [&] { kh_launch_read_lookup(rj, table, st); }); }));
        r0 += in.pivot_nreads[p];
    }
    *done = true;
    return KH_OK;
}
// What the set form and the index form share: the genomes' plain builds, the -cs{cs} union of every group with its
// histogram and `set_counts 1`, as exp4_sets makes them.  gsets.v[g] is what the votes are taken against.
struct Exp6Sets { SetBag plain, unions, gsets; };
static int exp6_group_sets(kh_ctx* c, const Exp6In& in, const Exp6Out& out, Exp6Sets* s) {
    const int nseq = in.nseq;
    KHCHK(build_plain(c, nseq, in.seqs, in.lens, 0, nullptr, nullptr, in.on_device, in.k, &s->plain));
    for (int i = 0; i < nseq; ++i)
        if (out.distinct_per_seq) out.distinct_per_seq[i] = s->plain.v[i]->n;
    KHCHK(group_unions(c, s->plain.v.data(), nseq, in.group_of, in.ngroups, in.cs, &s->unions, out.within_hist, in.hist_len));
    return group_ones(c, s->unions, &s->gsets);
}
// The index form (kh_index.hip): ONE merged mask index over the groups' sets, then per pivot the batches of
// read_votes_batches, whose masks k_read_index finds with one lookup per window.  No check set, as in the set form.
// KHOICE_EXP6_INDEX=1 takes the form whenever it applies, =0 never; unset follows the rule below.  *done == false: the
// form does not apply or was not chosen (nothing of it was launched), the set form answers:
//   * more groups than kh_read_votes takes (the set form reports them);
//   * the upper bound of the index, sum |sets| * (8 W + 8 mwords + 8 / B), plus the workspace of its union (the union's
//     counters, and above one launch's fan-in the partial unions) is above a quarter of the free memory, the budget of
//     reads_max_pos (KHOICE_INDEX_MAX_BYTES lowers it).
// The rule: the set form's work grows with windows * ngroups searches, the index adds a build that grows with
// sum |sets|, so the form is taken from windows * ngroups >= R * sum |sets| on.  Measured (tools/bench_exp6_index.py,
// profiles/exp6_index.json, DESIGN.md §3 "Merged mask index"): at 10 groups x 5 genomes x 5 Mbp the index wins every
// point from the ratio 0.5307 on (k = 63, 10 x 10 000 reads of 150 bases: 26 ms against 40 ms; 10 kb reads: 30 x) and
// loses at 0.10 and 0.01; R is that ratio rounded down.  The same ratios at small inputs: up to sum |sets| = 1.6e5 a
// call is 0.6 ms of launches and synchronisations either way and the index never wins, at 1.1e6 .. 1.5e6 it wins one
// point of three, from 3.6e6 on all of them: below that size the rule does not hold and the set form stays.
constexpr double KH_EXP6_INDEX_RATIO = 0.53;
constexpr u64 KH_EXP6_INDEX_MIN_KEYS = 3600000;
static int exp6_index(kh_ctx* c, const Exp6In& in, const Exp6Out& out, const SetBag& gsets, bool* done) {
    *done = false;
    const int ngroups = in.ngroups;
    const char* sw = getenv("KHOICE_EXP6_INDEX");
    const bool forced = sw && atoi(sw) != 0;
    if (sw && !forced) return KH_OK;
    if ((u32)ngroups > KH_READS_MAX_SETS) return KH_OK;
    u64 total = 0;
    for (const kh_set* s : gsets.v) total += s->n;
    if (!forced) {
        if (total < KH_EXP6_INDEX_MIN_KEYS) return KH_OK;
        double windows = 0;
        for (int p = 0; p < in.npivots; ++p) {
            if (!in.pivot_read_off[p]) return KH_OK;        // (the set form's call reports it)
            for (u64 i = 0; i < in.pivot_nreads[p]; ++i) {
                const u64 a = in.pivot_read_off[p][i], b = in.pivot_read_off[p][i + 1];
                if (b > a && b - 1 - a >= (u64)in.k) windows += (double)(b - 1 - a - (u64)in.k + 1);
            }
        }
        if (windows * (double)ngroups < KH_EXP6_INDEX_RATIO * (double)total) return KH_OK;
    }
    {   // ---- the memory budget
        const u64 W = in.k <= 32 ? 1 : 2, mwords = (u64)std::max(1, (ngroups + 63) / 64);
        u64 budget = 1ull << 30;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = (free_b + c->pool.cached_bytes) / 4;
        if (const char* e = getenv("KHOICE_INDEX_MAX_BYTES")) budget = std::min<u64>(budget, strtoull(e, nullptr, 10));
        const u64 need = total * (8 * W + 8 * mwords) + 8 * (total / index_bucket_keys() + 2)       // keys, masks, dir
                         + total * (4 + (ngroups > KH_MAX_INPUT_SETS ? 8 * W + 4 : 0))                // the union's workspace
                         + 8ull * (total / 16 + 2 * (u64)ngroups + 64);                               // (its bounds and descriptors)
        if (need > budget) return KH_OK;
    }
    struct Guard { kh_index* ix = nullptr; ~Guard() { kh_index_free(ix); } } g;
    KHCHK(kh_index_build(c, gsets.v.data(), ngroups, &g.ix));
    const u64 nwords = g.ix->mwords;
    u64 r0 = 0;
    for (int p = 0; p < in.npivots; ++p) {
        if (!in.pivot_read_off[p]) return kh_fail(KH_E_ARG, "kh_read_votes: NULL argument");   // (as the set form's call says it)
        KHCHK(read_votes_index(c, in.pivot_reads[p], in.pivot_read_off[p], in.pivot_nreads[p], in.on_device, g.ix, nullptr,
                               out.tie_masks ? out.tie_masks + r0 * nwords : nullptr, nullptr, out.unmatched ? out.unmatched + r0 : nullptr));
        r0 += in.pivot_nreads[p];
    }
    *done = true;
    return KH_OK;
}
// The set form: kh_read_votes per pivot's reads against the groups' sets.
static int exp6_sets(kh_ctx* c, const Exp6In& in, const Exp6Out& out, const SetBag& gsets) {
    const int ngroups = in.ngroups;
    const u64 nwords = (u64)std::max(1, (ngroups + 63) / 64);
    u64 r0 = 0;
    for (int p = 0; p < in.npivots; ++p) {
        KHCHK(kh_read_votes(c, in.pivot_reads[p], in.pivot_read_off[p], in.pivot_nreads[p], in.on_device, in.k, gsets.v.data(), ngroups,
                            nullptr, out.tie_masks ? out.tie_masks + r0 * nwords : nullptr, nullptr, out.unmatched ? out.unmatched + r0 : nullptr));
        r0 += in.pivot_nreads[p];
    }
    return KH_OK;
}
extern "C" int kh_exp6_run(kh_ctx* c, int nseq, const uint8_t* const* seqs, const uint64_t* lens, int on_device,
                           const int* group_of, int ngroups, int npivots, const uint8_t* const* pivot_reads,
                           const uint64_t* const* pivot_read_off, const uint64_t* pivot_nreads, int k, uint32_t cs,
                           uint64_t* within_hist, uint32_t hist_len, uint64_t* tie_masks, uint32_t* unmatched,
                           uint64_t* distinct_per_seq) {
    KHCHK(exp_check_args("kh_exp6_run", c, nseq, seqs, lens, group_of, ngroups, npivots, pivot_reads, pivot_read_off, false, nullptr,
                         hist_len, k, cs, nullptr));
    if (npivots && !pivot_nreads) return kh_fail(KH_E_ARG, "kh_exp6_run: bad argument");
    const Exp6In in{nseq, seqs, lens, on_device, group_of, ngroups, npivots, pivot_reads, pivot_read_off, pivot_nreads, k, cs, hist_len};
    const Exp6Out out{within_hist, tie_masks, unmatched, distinct_per_seq};
    HIPCHK(hipSetDevice(c->dev));
    bool done = false;
    KHCHK(exp6_bmp(c, in, out, &done));       // the order of the forms: bitmaps, index, sets
    if (done) return KH_OK;
    Exp6Sets s;
    KHCHK(exp6_group_sets(c, in, out, &s));
    KHCHK(exp6_index(c, in, out, s.gsets, &done));
    if (done) return KH_OK;
    return exp6_sets(c, in, out, s.gsets);
}

// ------------------------------------------------------------------------------ fused experiment type 3
struct Exp3In {   // the arguments of kh_exp3_run that both forms read
    int nseq; const uint8_t* const* seqs; const uint64_t* lens; int on_device;
    const int* group_of; int ngroups;
    int npivots; const uint8_t* const* pivot_seqs; const uint64_t* pivot_lens;
    int k; u32 cs, hist_len;
};
struct Exp3Out {   // any of them may be NULL
    uint64_t *inter_hist, *distinct_per_seq, *distinct_per_pivot;
    // occ k-mers of pivot p occur in v >= 1 genomes of group g: what `intersect -ocsum` with the -cs{cs} union, then
    // `transform histogram`, make of them (the fold of Exp2Out::add)
    void add(const Exp3In& in, int p, int g, u32 v, u64 occ) const {
        if (inter_hist)
            inter_hist[((size_t)p * in.ngroups + g) * in.hist_len + ocsum_bin(v, in.cs, in.hist_len)] += occ;
    }
    void clear(const Exp3In& in) const {
        if (inter_hist) memset(inter_hist, 0, 8 * (size_t)in.npivots * in.ngroups * in.hist_len);
        if (distinct_per_pivot) memset(distinct_per_pivot, 0, 8 * (size_t)in.npivots);
        if (distinct_per_seq) memset(distinct_per_seq, 0, 8 * (size_t)in.nseq);
    }
};
// The presence-bitmap form (kh_bmp.hip): genomes (group-major) and pivots are the operands of the unchanged
// k_bmp_build; k_bmp_cross counts a batch of pivots against the bit-sliced counter of every group, one launch and one
// zeroed block of replicas per batch.  A batch holds as many pivots as fit the bins (KH_BMP_MAX_BINS, lowered by
// KHOICE_BMP_MAX_BINS) and the LDS kept for their words (KH_BMP_CROSS_PIVOTS).  *done == false: the form does not apply
// (nothing was launched, no retry is counted).
static int exp3_bmp(kh_ctx* c, const Exp3In& in, const Exp3Out& out, bool* done) {
    *done = false;
    const int k = in.k, nseq = in.nseq, ngroups = in.ngroups, npiv = in.npivots;
    if (!bmp_form_k(k)) return KH_OK;
    // ---- operands: the genomes in group-major order, then the pivots
    const BmpOperands o = bmp_operands(nseq, in.seqs, in.lens, in.group_of, ngroups, npiv, in.pivot_seqs, in.pivot_lens);
    std::vector<KhBmpGroup> groups(ngroups);
    for (int g = 0; g < ngroups; ++g) {
        if (o.size[g] > KH_BMP_MAX_COUNT) return KH_OK;
        groups[g] = KhBmpGroup{o.first[g], o.size[g], o.first[g], 0};   // (a pivot has one bin per genome: count v of group g at bin0 + v - 1)
    }
    u64 max_bins = KH_BMP_MAX_BINS;
    if (const char* e = getenv("KHOICE_BMP_MAX_BINS")) max_bins = std::min<u64>(max_bins, strtoull(e, nullptr, 10));
    // a launch of np pivots: np * nseq bins and np + nseq distinct counters
    if ((u64)nseq + (npiv ? (u64)nseq + 1 : 0) > max_bins) return KH_OK;
    const u32 batch = npiv ? (u32)std::min<u64>(std::min<u64>((max_bins - (u64)nseq) / ((u64)nseq + 1), KH_BMP_CROSS_PIVOTS), (u64)npiv) : 0;
    const u32 nbatches = npiv ? ((u32)npiv + batch - 1) / batch : 1;
    // ---- the batches' blocks of replicas count against the budget of the partial bitmaps, in rows of one bitmap
    const u32 nb_max = batch * (u32)nseq + batch + (u32)nseq;   // bins and counters of a full batch
    const u64 nwords = k >= 3 ? 1ull << (2 * k - 6) : 1;
    const u64 extra_rows = ((u64)nbatches * BmpRun::reps_max(nb_max) * nb_max + nwords - 1) / nwords;
    BmpRun run(c, k, in.on_device, o);
    bool fits = false;
    KHCHK(run.plan(extra_rows, &fits));
    if (!fits) return KH_OK;
    run.layout(nbatches, nb_max);
    const size_t off_groups = run.table(groups);
    KHCHK(run.upload());
    KHCHK(run.build());
    KhBmpCrossJob job{};
    job.ops = run.ops();
    job.groups = run.dev<const KhBmpGroup>(off_groups);
    job.partial = run.d_partial.as<u64>();
    job.nwords = run.s.nwords;
    job.ngenomes = (u32)nseq; job.ngroups = (u32)ngroups; job.reps = run.reps;
    for (u32 b = 0; b < nbatches; ++b) {
        job.pop0 = (u32)nseq + b * batch;
        job.npivots = std::min<u32>(batch, (u32)npiv - b * batch);   // (no pivots: one launch for the genomes' counters)
        job.nbins = job.npivots * (u32)nseq;
        job.hist = run.hist(b);
        KHCHK(timed_launch(c, KC_BMP_CROSS, [&] { kh_launch_bmp_cross(job, run.s.rgrid, run.s.rwaves, c->st); }));
    }
    KHCHK(run.download());

    // ---- per batch the bins folded; the genomes' counters from the first batch
    out.clear(in);
    u64 dsum = 0, met = 0;
    std::vector<u64> bins;
    for (u32 b = 0; b < nbatches; ++b) {
        const u32 p0 = b * batch, np = std::min<u32>(batch, (u32)npiv - p0), nbins = np * (u32)nseq;
        run.bins(b, nbins + np + (u32)nseq, &bins);
        if (b == 0)
            for (int i = 0; i < nseq; ++i) {
                const u64 d = bins[nbins + np + o.op_of_seq[i]];
                dsum += d;
                if (out.distinct_per_seq) out.distinct_per_seq[i] = d;
            }
        for (u32 q = 0; q < np; ++q) {
            dsum += bins[nbins + q];
            if (out.distinct_per_pivot) out.distinct_per_pivot[p0 + q] = bins[nbins + q];
            for (int g = 0; g < ngroups; ++g)
                for (u32 v = 1; v <= groups[g].size; ++v) {
                    const u64 occ = bins[(size_t)q * nseq + groups[g].bin0 + v - 1];
                    met += occ;
                    out.add(in, (int)(p0 + q), g, v, occ);
                }
        }
    }
    run.account(dsum, met);   // pivot k-mers met in a group, summed over the groups
    *done = true;
    return KH_OK;
}
// The super-k-mer form (k_skm_cross, kh_skm_device.h; k = 17 .. 63, taken only with KHOICE_EXP3_SKM=1 — the set form
// stays the default until the form has been measured): genomes and pivots go through the unchanged scatter and regroup
// as ONE list of texts, the pivots behind the genomes and every pivot a group of its own (TagLayout: its tag is then
// nseq + q; a read set's line feeds are non-bases to the scatter).  One direct launch walks all slots, a listed one
// the slots whose region overflowed.  At most 64 operands a pass: more pivots than 64 - nseq go in batches, every
// batch with the genomes staged, scattered and walked AGAIN (wasteful, known: a pass that keeps the genomes' records
// is what would mend it); the genomes' distinct counts are the first pass's.  *done == false and no retry counted: the
// form does not apply (switch, k, KHOICE_NO_SKM / KHOICE_NO_SKM2, no pivot — the set form builds the genomes only —,
// more than 63 genomes, no k-mer position, geometry, memory), nothing of the outputs was written.  A capacity or order
// error of a kernel, or more spilled records or listed slots than are kept: retries++, and the set form answers.
static int exp3_skm(kh_ctx* c, const Exp3In& in, const Exp3Out& out, bool* done) {
    *done = false;
    const int k = in.k, nseq = in.nseq, ngroups = in.ngroups, npiv = in.npivots;
    const char* sw = getenv("KHOICE_EXP3_SKM");
    if (!sw || atoi(sw) != 1 || !skm_form_k(k)) return KH_OK;
    if (!npiv || nseq >= KH_TAG_MAX_OPS) return KH_OK;
    const int batch = std::min(npiv, KH_TAG_MAX_OPS - nseq), nbatches = (npiv + batch - 1) / batch;
    u64 gbases = 0, pbases = 0;
    const u64 gpos = kmer_positions(nseq, in.lens, k, &gbases);
    for (int b = 0; b < nbatches; ++b)   // (a pass without a k-mer position has no geometry)
        if (!(gpos + kmer_positions(std::min(batch, npiv - b * batch), in.pivot_lens + (size_t)b * batch, k))) return KH_OK;
    kmer_positions(npiv, in.pivot_lens, k, &pbases);
    const KhSkmWidth& wd = kh_skm_width(k > KH_SKM_MAX_K);
    u32 fan = 1;
    {
        std::vector<u32> gs(ngroups, 0);
        for (int i = 0; i < nseq; ++i) fan = std::max(fan, ++gs[in.group_of[i]]);
    }
    std::vector<u64> dseq(nseq, 0), dpiv(npiv, 0), occ((size_t)npiv * nseq, 0);   // occ[p][first genome of g + v - 1]
    std::vector<int> gstart, gsize;
    u64 kmers = 0, records = 0, multi = 0, big = 0;
    for (int b = 0; b < nbatches; ++b) {
        const int p0 = b * batch, np = std::min(batch, npiv - p0), nops = nseq + np;
        std::vector<const uint8_t*> seqs(in.seqs, in.seqs + nseq);
        std::vector<uint64_t> lens(in.lens, in.lens + nseq);
        std::vector<int> group_of(in.group_of, in.group_of + nseq);
        for (int q = 0; q < np; ++q) {
            seqs.push_back(in.pivot_seqs[p0 + q]);
            lens.push_back(in.pivot_lens[p0 + q]);
            group_of.push_back(ngroups + q);
        }
        SkmRun s(c);
        // fan hint: a pivot's reads bring copies of their locus into the slot of the group they were drawn from — one
        // more than the largest group.  A guess (reads may cover a locus many times); the side list takes what it misses.
        KHCHK(skm_prepare(c, nops, seqs.data(), lens.data(), in.on_device, group_of.data(), ngroups + np, k, false, 0, fan + 1, &s, wd.cross_round));
        if (!s.staged) {
            if (b) c->stat.retries++;   // (a later pass whose geometry or memory does not fit: work was done for nothing)
            return KH_OK;
        }
        const TagLayout& L = s.L;
        const KhSkmJob& job = s.job;
        hipStream_t st = c->st;
        KhSkmCrossJob cj{};
        cj.ngenomes = (u32)nseq;
        cj.nbins = (u32)np * (u32)nseq;
        const u64 pm = (np >= 64 ? ~0ull : (1ull << np) - 1ull) << nseq;
        cj.pmlo = (u32)pm; cj.pmhi = (u32)(pm >> 32);
        const u32 grid = std::min<u32>(s.g.nslots, wd.cross_per_cu * (u32)std::max(1, c->cus));
        cj.reps = std::min<u32>(grid, 64);
        const size_t bins_bytes = 8 * (size_t)cj.reps * cj.nbins;
        Tmp d_bins;
        TMP_ALLOC(d_bins, c, bins_bytes);
        Pinned pin{c};
        PIN_ALLOC(pin, bins_bytes);
        cj.bins = d_bins.as<unsigned long long>();
        HIPCHK(hipMemsetAsync(cj.bins, 0, bins_bytes, st));
        KHCHK(timed_launch(c, KC_SKM_CROSS, [&] { wd.cross(job, cj, grid, st); }));
        bool declines = false;
        KHCHK(s.settle(s.off.ctl, [&](u32 nlisted) {   // ([ctl .. dup] of the workspace; the bins are read back below)
            big += nlisted;
            cj.nlisted = nlisted;
            return timed_launch(c, KC_SKM_CROSS, [&] { wd.cross(job, cj, nlisted, st); });
        }, &declines));
        if (declines) return KH_OK;   // the set form takes over
        HIPCHK(hipMemcpyAsync(pin.p, cj.bins, bins_bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        records += s.h_ctl()[KH_SKM_CTL_RECORDS];
        multi += s.h_ctl()[KH_SKM_CTL_MULTI];
        s.per_text([&](int t, u64 inst, u64 d) {   // text t of this pass: the genomes, then its pivots
            if (t >= nseq) { dpiv[p0 + t - nseq] = d; kmers += inst; }
            else if (b == 0) { dseq[t] = d; kmers += inst; }
        });
        const u64* h_bins = static_cast<const u64*>(pin.p);
        for (u32 r = 0; r < cj.reps; ++r)
            for (int q = 0; q < np; ++q)
                for (int j = 0; j < nseq; ++j) occ[(size_t)(p0 + q) * nseq + j] += h_bins[(size_t)r * cj.nbins + (size_t)q * nseq + j];
        if (b == 0) {
            gstart.assign(L.gstart.begin(), L.gstart.begin() + ngroups);
            gsize.assign(L.gsize.begin(), L.gsize.begin() + ngroups);
        }
    }
    // ---- every pass went through: the outputs, and the accounting of exp3_bmp
    out.clear(in);
    u64 dsum = 0, met = 0;
    for (int i = 0; i < nseq; ++i) {
        dsum += dseq[i];
        if (out.distinct_per_seq) out.distinct_per_seq[i] = dseq[i];
    }
    for (int p = 0; p < npiv; ++p) {
        dsum += dpiv[p];
        if (out.distinct_per_pivot) out.distinct_per_pivot[p] = dpiv[p];
        for (int g = 0; g < ngroups; ++g)
            for (int v = 1; v <= gsize[g]; ++v) {
                const u64 n = occ[(size_t)p * nseq + gstart[g] + v - 1];
                met += n;
                out.add(in, p, g, (u32)v, n);
            }
    }
    c->stat.skm_records += records;
    c->stat.cross_multi_slots += multi;
    c->stat.big_slots += big;
    c->stat.bases += gbases + pbases;
    c->stat.builds += (u64)nseq + (u64)npiv;
    c->stat.kmers += kmers;
    c->stat.distinct += dsum;
    c->stat.setop_in += dsum;
    c->stat.setop_out += met;   // pivot k-mers met in a group, summed over the groups
    c->stat.setops++;
    *done = true;
    return KH_OK;
}
// The set form: the calls of workflow/exp_type_3.py::run_batched on sets that stay in device memory — one batched plain
// build of genomes and pivots, the -cs{cs} union of every group, and intersect -ocsum + histogram of every pivot with
// every union.  No kernel of its own.
static int exp3_sets(kh_ctx* c, const Exp3In& in, const Exp3Out& out) {
    const int nseq = in.nseq, ngroups = in.ngroups, npiv = in.npivots;
    SetBag plain, unions;   // every intermediate set, freed on every way out
    KHCHK(build_plain(c, nseq, in.seqs, in.lens, npiv, in.pivot_seqs, in.pivot_lens, in.on_device, in.k, &plain));
    out.clear(in);
    for (int i = 0; i < nseq; ++i)
        if (out.distinct_per_seq) out.distinct_per_seq[i] = plain.v[i]->n;
    for (int p = 0; p < npiv; ++p)
        if (out.distinct_per_pivot) out.distinct_per_pivot[p] = plain.v[nseq + p]->n;
    if (!out.inter_hist || !npiv) return KH_OK;
    KHCHK(group_unions(c, plain.v.data(), nseq, in.group_of, ngroups, in.cs, &unions, nullptr, 0));
    for (int p = 0; p < npiv; ++p)
        for (int g = 0; g < ngroups; ++g) {
            SetBag r;
            KHCHK(kh_simple(c, plain.v[nseq + p], unions.v[g], KH_INTERSECT, KH_MODE_SUM, in.cs, r.slot()));
            KHCHK(kh_histogram(c, r.v[0], out.inter_hist + ((size_t)p * ngroups + g) * in.hist_len, in.hist_len));
        }
    return KH_OK;
}
extern "C" int kh_exp3_run(kh_ctx* c, int nseq, const uint8_t* const* seqs, const uint64_t* lens, int on_device,
                           const int* group_of, int ngroups, int npivots, const uint8_t* const* pivot_seqs,
                           const uint64_t* pivot_lens, int k, uint32_t cs, uint64_t* inter_hist, uint32_t hist_len,
                           uint64_t* distinct_per_seq, uint64_t* distinct_per_pivot) {
    KHCHK(exp_check_args("kh_exp3_run", c, nseq, seqs, lens, group_of, ngroups, npivots, pivot_seqs, pivot_lens, false, nullptr,
                         hist_len, k, cs, nullptr));
    const Exp3In in{nseq, seqs, lens, on_device, group_of, ngroups, npivots, pivot_seqs, pivot_lens, k, cs, hist_len};
    const Exp3Out out{inter_hist, distinct_per_seq, distinct_per_pivot};
    HIPCHK(hipSetDevice(c->dev));
    bool done = false;
    KHCHK(exp3_bmp(c, in, out, &done));
    if (done) return KH_OK;
    KHCHK(exp3_skm(c, in, out, &done));   // (KHOICE_EXP3_SKM=1 only)
    if (done) return KH_OK;
    return exp3_sets(c, in, out);
}

// ------------------------------------------------------------------------------ host mix
extern "C" void kh_mix_host(int k, const uint64_t* in, uint64_t* out) {
    if (k <= 32) {
        KmerKey<1> a{in[0]};
        a = kh_mix(a, k);
        out[0] = a.lo;
    } else {
        KmerKey<2> a{in[0], in[1]};
        a = kh_mix(a, k);
        out[0] = a.lo;
        out[1] = a.hi;
    }
}
extern "C" void kh_unmix_host(int k, const uint64_t* in, uint64_t* out) {
    if (k <= 32) {
        KmerKey<1> a{in[0]};
        a = kh_unmix(a, k);
        out[0] = a.lo;
    } else {
        KmerKey<2> a{in[0], in[1]};
        a = kh_unmix(a, k);
        out[0] = a.lo;
        out[1] = a.hi;
    }
}
