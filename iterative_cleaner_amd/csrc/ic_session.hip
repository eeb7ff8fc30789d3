// ic_session.hip — host side of libicgpu.so: the C-ABI declared in
// include/iterative_cleaner.h.  Owns device buffers and the HIP stream of a
// session, prepares the fit cube at the start of every run, and drives the cleaning
// loop of iterative_cleaner.py:83-146 (one launch sequence per iteration and
// one small device->host read of the convergence counters).  A channel shard
// (ic_session_create_shard / _grouped) runs the same sequence on its channel
// slice with four exchanges per iteration through a Comm (ic_comm.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <stdio.h>
#include <sched.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/iterative_cleaner.h"
#include "ic_comm.h"
#include "ic_internal.h"

using namespace icgpu;

namespace icgpu {
thread_local PendingTiming g_timing;
}

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// calls on a session whose host wait timed out (Session::failed)
int failed_session()
{
    return fail(IC_ESTATE, "session failed: a host wait timed out with its kernels possibly still running; destroy it");
}

#define CK(call)                                                                                  \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(IC_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                                \
    } while (0)

// the entry points that report a HIP error under their own name (`bad`: the
// error -> their return code)
#define CKF(call, bad)                        \
    do {                                      \
        const hipError_t e_ = (call);         \
        if (e_ != hipSuccess) return bad(e_); \
    } while (0)

int named_fail(const char *name, hipError_t e, bool oom_is_enomem = false)
{
    if (oom_is_enomem && e == hipErrorOutOfMemory) return fail(IC_ENOMEM, "%s: device allocation failed", name);
    return fail(IC_EHIP, "%s: %s", name, hipGetErrorString(e));
}

// The owner of device buffers: every hipMalloc and hipFree of this file.  A
// buffer is added with one alloc() line and freed with its arena.  Buffers
// are registered by value, not by the address of the pointer handed in: the
// session swaps and aliases its pointers.
struct DeviceArena {
    std::vector<void *> bufs;
    DeviceArena() = default;
    DeviceArena(const DeviceArena &) = delete;
    DeviceArena &operator=(const DeviceArena &) = delete;
    ~DeviceArena() { free_all(); }
    hipError_t alloc_bytes(void **p, size_t bytes)
    {
        const hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess) *p = nullptr;
        else if (*p) bufs.push_back(*p);
        return e;
    }
    // n elements + 16 bytes of padding; exact: no padding (the delays, the per-call
    // buffers); ensure: a buffer allocated at first need
    template <typename T> hipError_t alloc(T **p, size_t n) { return alloc_bytes((void **)p, n * sizeof(T) + 16); }
    template <typename T> hipError_t alloc_exact(T **p, size_t n) { return alloc_bytes((void **)p, n * sizeof(T)); }
    template <typename T> hipError_t ensure(T **p, size_t n) { return *p ? hipSuccess : alloc(p, n); }
    template <typename T> void release(T *&p)   // one buffer, early
    {
        const auto it = std::find(bufs.begin(), bufs.end(), (void *)p);
        if (it != bufs.end()) {
            (void)hipFree(*it);
            bufs.erase(it);
        }
        p = nullptr;
    }
    void free_all()
    {
        for (void *b : bufs) (void)hipFree(b);
        bufs.clear();
    }
    void abandon() { bufs.clear(); }   // leak on purpose (a failed session's buffers may be in use)
};

// The one-shot entry points' buffers and private stream, and per-call
// temporaries of a session: gone when the call returns, on every path.
struct Scratch {
    DeviceArena mem;
    hipStream_t stream = nullptr;
    hipError_t open_stream() { return hipStreamCreateWithFlags(&stream, hipStreamNonBlocking); }
    ~Scratch()
    {
        mem.free_all();
        if (stream) (void)hipStreamDestroy(stream);
    }
};

int select_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(IC_EHIP, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(IC_EINVAL, "device %d out of range (%d devices)", device, ndev);
    CK(hipSetDevice(device));
    return IC_OK;
}

int check_q_flags(int flags)
{
    if (flags & ~IC_Q_BIG_ENDIAN) return fail(IC_EINVAL, "unknown flag bits 0x%x", (unsigned)(flags & ~IC_Q_BIG_ENDIAN));
    return IC_OK;
}

const char *kKernelNames[K_COUNT] = {"k_chan_partials", "k_window",    "k_base",
                                     "k_fscrunch",      "k_tscrunch",  "k_fit_pass", "k_fit_state",
                                     "k_diag",          "k_linestats", "k_combine",  "k_residual",
                                     "k_fit_tail",      "k_sb_tree",   "k_shard_pack", "exchange",
                                     "k_tnorm",         "k_rotate",    "k_residual_q", "k_std_align",
                                     "k_std_install",   "k_hotbins",   "k_hotbin_scan", "k_dynspec"};

constexpr long kTailProfiles = 8192;  // default: hand the remaining profiles to k_fit_tail below this
constexpr long kTailProfilesLarge = 4096;   // the same for sessions of >= 2^20 profiles
constexpr long kTailProfilesLong = 12288;   // smaller sessions of >= 2048-bin profiles

struct Timed {
    int kid;
    hipEvent_t a, b;
};

struct Session {
    ic_params p{};
    int device = 0;
    hipStream_t stream = nullptr;
    size_t P = 0, N = 0, Ppad = 0;
    int ldD = 0;                // fit-cube row stride (bins, padded to kFitTile)
    int nsb = 0, width = 0;
    bool uploaded = false, ran = false;
    int last_iter = 0;
    // channel shard (unsharded: world == 1, comm == nullptr, nchan == p.nchan)
    int rank = 0, world = 1;
    Comm *comm = nullptr;
    int nchan = 0;                  // channels of this session (local slice)
    int c0 = 0;                     // its first global channel
    ShardGeom geom{};
    SbPlan plan_sb{};               // the session's super-blocks
    SbPlan plan_top{};              // the shard roots (world leaves)
    int rows_own = 0, rows_pad = 0;
    double *xw_send = nullptr, *xw_recv = nullptr;          // window-total roots -> row owners
    double *xf_send = nullptr, *xf_recv = nullptr;          // fscrunch + weight roots -> row owners
    int32_t *xwg_send = nullptr, *xwg_recv = nullptr;       // owners' windows, all-gathered
    float *xfg_send = nullptr, *xfg_recv = nullptr;         // owners' fscrunch rows, all-gathered
    int wg_blk = 0;                                          // ints per rank in xwg (rows_pad, even)
    long fg_blk = 0;                                         // floats per rank in xfg (even)
    std::vector<size_t> wsb, wrb, fsb, frb;                 // block bytes: window / fscrunch roots
    unsigned char *xd_send = nullptr, *xd_recv = nullptr;   // diagnostics / valid rows
    double *xr_send = nullptr, *xr_recv = nullptr;          // row medians / MADs
    std::vector<size_t> dsb, drb, vsb, vrb;                 // block bytes: diag, valid
    double *std_r = nullptr, *mean_r = nullptr, *fft_r = nullptr;   // owned rows [rows_own][nchan_g]
    double *ptp_r = nullptr;
    uint8_t *valid_r = nullptr;
    // device buffers: owned by `mem`, but for the exchange buffers and a shard's
    // counters (the transport's: comm->alloc / comm->release)
    DeviceArena mem;
    float *raw = nullptr, *D = nullptr, *w0 = nullptr, *W = nullptr, *base = nullptr, *base0 = nullptr;
    // input slots (raw/w0/shift alias slot `cur`); slot 1 is allocated by the first
    // ic_upload_async that needs it.  Pending async uploads queue in `fifo`.
    float *slot_raw[2] = {nullptr, nullptr}, *slot_w0[2] = {nullptr, nullptr};
    int32_t *slot_shift[2] = {nullptr, nullptr};
    hipEvent_t slot_ev[2] = {nullptr, nullptr};
    // quantised uploads (ic_upload_quantised*): per input slot the int16 samples
    // [nsub][nsum][nchan][nbin] and scl then offs [nsub][nsum][nchan] each, decoded
    // into slot_raw; allocated by the first such upload into the slot for its nsum
    // (slot_qsum), regrown for a larger one
    int16_t *slot_q[2] = {nullptr, nullptr};
    float *slot_so[2] = {nullptr, nullptr};
    int slot_qsum[2] = {0, 0};
    // quantised download (ic_get_residual_quantised): the encoded residual's
    // int16 samples [N] and scl then offs [P] each; first use, kept
    int16_t *res_q = nullptr;
    float *res_so = nullptr;
    // its asynchronous form (ic_get_residual_quantised_async): the copies run on
    // dl_stream (first use; neither the session's stream nor copy_stream, so
    // downloads, uploads and cleaning queue behind nothing but their own kind).
    // enc_ev: the encode is done (the session's stream); dl_ev: the newest
    // download has landed; dl_pending: dl_ev has not been waited for by the host;
    // enc_slot: the input slot the newest encode read (raw, shift), -1 once an
    // upload into it has been ordered behind enc_ev
    hipStream_t dl_stream = nullptr;
    hipEvent_t enc_ev = nullptr, dl_ev = nullptr;
    bool dl_pending = false;
    int enc_slot = -1;
    hipStream_t copy_stream = nullptr;
    int cur = 0, fifo[2] = {0, 0}, fifo_n = 0;
    bool ever_uploaded = false;
    float *F = nullptr, *wf = nullptr, *T = nullptr, *hist = nullptr;
    double *ptp = nullptr;      // f64 storage; f32 values unless p.data_f64
    uint8_t *valid = nullptr;
    int32_t *shift = nullptr, *win = nullptr, *wflag = nullptr, *info = nullptr, *counters = nullptr;
    double *part = nullptr, *part2 = nullptr, *wpart = nullptr, *T64 = nullptr, *amp = nullptr, *std_ = nullptr,
           *mean = nullptr, *fft = nullptr, *test = nullptr, *lstat = nullptr, *TT = nullptr,
           *T2 = nullptr;   // [2 nbin]: the template twice (k_diag_cl)
    double2 *tw = nullptr, *tw_p2 = nullptr;
    PwPlan *plan = nullptr;
    FitStateArrays fs{};
    int32_t *lists = nullptr;   // two active-profile lists of P entries
    int32_t *rcount = nullptr;  // round counters (ic_internal.h kRoundWords) + the tail's sweep counter
    int32_t *h_rcount = nullptr;  // host-mapped mirror, written by k_fit_state's last block
    int32_t *h_small = nullptr;   // pinned readback of the per-iteration counters and run stats
                                  // (a pageable D2H copy is staged synchronously, ~30 us each)
    int32_t *d_h_rcount = nullptr;  // its device address
    void *fs_block = nullptr;   // one allocation backing fs
    int fit_rounds = 0;
    int plan_ub = 0;            // max(leaves, ops) of the pairwise plan (k_tnorm scratch)
    LineStatsArgs ls_knobs;     // row-median form (IC_OPT_ROWSTAT_*)
    // detrended scaling (ic_set_detrend; both orders 0 = off: k_linestats and
    // k_combine as ever, no buffer).  trend: [4][nchan][4] channel then
    // [4][nsub][4] subint coefficients, from `mem` at the first detrended run;
    // trends_ran: the last run's last iteration wrote them
    int dt_chan = 0, dt_sub = 0, dt_rounds = 4;
    double dt_clip = 5.0;
    double *trend = nullptr;
    bool trends_ran = false;
    // piecewise detrending (ic_set_detrend_pieces): pw_on selects k_linetrend_pw /
    // k_combine_pw for detrended runs; pw_cs / pw_ss: the starts of a channel
    // line's / a subint line's pieces ({0}: one piece).  The device copies
    // (pw_starts: both lists, each closed by its n; pw_piece: the piece of every
    // subint, then of every channel; pw_trend: [4][nchan][mc][4] then
    // [4][nsub][ms][4]) come from `mem` at the first run after a change
    bool pw_on = false;
    std::vector<int32_t> pw_cs{0}, pw_ss{0};
    int32_t *pw_starts = nullptr;
    int16_t *pw_piece = nullptr;
    double *pw_trend = nullptr;
    // detrending on a channel shard (ic_shard_enable_detrend): sh_dt makes the
    // setters legal; there the subint pieces (pw_ss, the row half of pw_starts /
    // pw_piece) are those of the archive's whole subint lines (p.nchan entries),
    // the channel coefficients the shard's channels', the subint coefficients all
    // nsub rows'.  xt_send / xt_recv: the owner's slot of detrended row statistics
    // (rows_pad * (8 + 16 ms) doubles: med, MAD, coefficients) and the world
    // slots gathered; the transport's, from the first detrended run after
    // enabling or after a piece change (xt_ms: the ms they were sized for)
    bool sh_dt = false;
    double *xt_send = nullptr, *xt_recv = nullptr;
    size_t xt_ms = 0;
    // standard template (ic_set_std_template; std_template.py): std_on selects the
    // one-pass loop that fits against the supplied profile.  std_S: the standard
    // as given [nbin]; std_rot: its rotated copy (frac); std_c: the
    // cross-correlation [nbin]; std_rec: k_std_peak's record.  All from `mem` at
    // the first set, kept across uploads; std_mean: the mean of f64(S), summed in
    // ascending index when it is set; std_hash: 30 bits of the standard's samples
    // and mode (a shard's ranks compare them); std_ran: the last run aligned
    bool std_on = false, std_ran = false;
    int std_mode = IC_ALIGN_NONE;
    double std_mean = 0.0;
    uint32_t std_hash = 0;
    float *std_S = nullptr, *std_rot = nullptr;
    double *std_c = nullptr;
    StdAlignRec *std_rec = nullptr;
    // hot-bin repair (ic_set_hotbins; hotbins.py): hb_on queues k_hotbins at the
    // start of the first ic_run after an upload, before anything reads the cube
    // (hb_done: this upload has had its pass; hb_have: the counts, masks and row
    // starts below are this upload's).  hb_count [P], hb_mask [P][words], hb_offs
    // [P], hb_total [1], then the scan's block sums: from `mem` at the first pass, kept.
    // The profiles' offsets come from shift, or from the session's own delays:
    // delay2, or the channel row in dly while delay2 is null
    bool hb_on = false, hb_done = false, hb_have = false;
    double hb_thr = 0.0;
    int hb_start = 0, hb_end = 0, hb_rounds = 4;
    int32_t *hb_count = nullptr;
    uint32_t *hb_mask = nullptr;
    int64_t *hb_offs = nullptr, *hb_total = nullptr;
    // dynamic spectrum (ic_get_dynspec; dynspec.py): nothing of it runs in
    // ic_run.  ds_tt [2 + nbin]: mT, Stt and the table t of the template;
    // ds_out [3 P]: amp, err, base.  From `mem` at the first call, kept
    double *ds_tt = nullptr, *ds_out = nullptr;
    long tail_threshold = kTailProfiles;   // IC_OPT_FIT_TAIL
    bool diag_chain = true;     // IC_OPT_DIAG_CHAIN: k_diag_cl at nbin 1024/2048/4096
    int grid_cap = 0;           // IC_OPT_GRID_CAP: > 0 caps the grids of the grid-stride kernels
    double sync_timeout_s = 600.0;   // IC_OPT_SYNC_TIMEOUT_MS
    // a host wait timed out with kernels of this session possibly still in
    // flight: every later call but ic_session_destroy fails (IC_ESTATE), and
    // destroy leaks the device buffers instead of freeing memory in use
    bool failed = false;
    bool comm_lost = false;   // ... because the transport reported a lost peer
    // diagnostics forked onto a second stream (exact fit): the state kernel
    // of round diag_fork (0 = off) flags the profiles still fitting; from
    // round diag_fork + fork_delay on the others are measured on dstream while
    // the fit's latency-bound late rounds and tail run, the flagged ones on
    // the main stream once the fit is done.  C2, one MI355X, same box (ms per
    // clean): no fork 28.70-28.77, fork 3 / delay 1 27.99-28.06, 3 / 0
    // 28.53-28.61, 3 / 2 28.41-28.46, 4 / 0 28.01-28.19, 4 / 1 28.45-28.52
    int diag_fork = 3;
    int pr_lo = 0, pr_hi = 0;   // this run's clamped pulse region (the FFT mode's forked residual rotation)
    // incremental template stage (integer dedispersion, iteration >= 2):
    // column exactness flags [nsub][nsb][nbin] of part (exA, set once per run
    // by prepare) and part2 (exF, set by every full fscrunch pass);
    // k_chan_delta then moves the sums through the changed channels only
    bool incr = true;
    uint8_t *exA = nullptr, *exF = nullptr;
    hipStream_t dstream = nullptr;
    hipEvent_t fork_ev = nullptr, join_ev = nullptr;
    uint8_t *late = nullptr;       // [P] 1: still fitting after round diag_fork (pass A skips them)
    int fork_round = -1;           // this iteration's fork round (-1: none)
    // the second fork (run_fit): the tail's list, marked in tmark, measured after the fit
    bool tail_split = false;
    // FFT mode: the residual's rotation measures its rows itself (k_rotate's
    // statistics epilogue, nbin 1024) instead of a k_diag STATS pass over R
    // (IC_OPT_ROT_STATS)
    bool rot_stats = true;
    int tail_split_mode = IC_TAIL_SPLIT_AUTO;   // IC_OPT_TAIL_SPLIT
    const int32_t *tail_list = nullptr;
    const unsigned long long *tail_cin = nullptr;
    long tail_bound = 0;
    uint8_t *tmark = nullptr;
    hipEvent_t fork2_ev = nullptr;
    int fork_delay = 1;            // rounds between the flags and pass A (IC_OPT_FORK_DELAY)
    ic_run_stats stats{};
    std::vector<int32_t> bad_fits;   // per iteration of the last run: fit statuses outside 1-4
    // fractional dedispersion (dedisp_mode IC_DEDISP_FFT): the dedispersed raw
    // cube rot(raw), the template stage's rot(f32(raw - base)) (carried rows),
    // the residual scratch, zero shifts/levels for the shift-indexed kernels,
    // and the phasor table [nchan][nbin/2 + 1] of ic_set_delays
    bool fftded = false, delays_set = false;
    int dtiled = 0;                  // fit cube D in the tiled layout (dt_ofs)
    float *dr = nullptr, *Tc = nullptr, *R = nullptr, *zbase = nullptr;
    int32_t *zshift = nullptr;
    float *ph = nullptr;   // f32 pairs
    float *czt = nullptr;  // IC_DEDISP_FFT_ANY at a chirp-z length: the per-length tables (czt_tables)
    double2 *dczt = nullptr;   // diag_czt_supported(nbin): k_diag_czt's per-length tables (diag_czt_tables)
    double *dly = nullptr;           // [P] the session's delays on the device (first need): the channel
                                     // row k_phasor_table reads, or the per-profile delays
    double *delay2 = nullptr;        // = dly while per-profile delays are in force, else nullptr
    // delays attached to an asynchronous upload (ic_upload_delays_async), per
    // input slot: the delays [P] as copied (slot_dly), the channel table built
    // from them on the copy stream (slot_ph; slot_dmode 1) or nothing more
    // (per profile; 2).  0: the slot's upload carries no delays.  Buffers at
    // first need.  The ic_run that consumes the upload exchanges the slot's
    // buffers with the session's (ph and dly, or dly): the delays stay the session's own
    // when a later upload, attached or not, reuses the slot.
    float *slot_ph[2] = {nullptr, nullptr};
    double *slot_dly[2] = {nullptr, nullptr};
    int slot_dmode[2] = {0, 0};
    // timing
    bool timing = false;
    int timing_only = -1;            // >= 0: time only this kernel id
    std::vector<Timed> events;
    std::vector<hipEvent_t> epool;   // reused across runs: no hipEventCreate in the timed region
    hipEvent_t sev = nullptr;        // spin_sync's marker
    size_t enext = 0;
    double kms[K_COUNT] = {0};
    int klaunch[K_COUNT] = {0};
};

// numpy pairwise plan (loops_utils.h.src): leaves <= 128 in address order
int plan_build(std::vector<int> &ls, std::vector<int> &ll, std::vector<int> &oa, std::vector<int> &ob,
               int start, int n)
{
    if (n <= 128) {
        ls.push_back(start);
        ll.push_back(n);
        return (int)ls.size() - 1;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    const int a = plan_build(ls, ll, oa, ob, start, n2);
    const int b = plan_build(ls, ll, oa, ob, start + n2, n - n2);
    oa.push_back(a);
    ob.push_back(b);
    return -(int)oa.size();  // op o encoded as -(o+1)
}

int make_plan(int n, PwPlan *pl)
{
    std::vector<int> ls, ll, oa, ob;
    const int root = plan_build(ls, ll, oa, ob, 0, n);
    if ((int)ls.size() > kMaxLeaves || (int)oa.size() > kMaxLeaves) return -1;
    memset(pl, 0, sizeof *pl);
    pl->n = n;
    pl->nleaf = (int)ls.size();
    pl->nops = (int)oa.size();
    auto slot = [&](int id) { return id >= 0 ? id : pl->nleaf + (-id - 1); };
    for (int q = 0; q < pl->nleaf; ++q) {
        pl->leaf_start[q] = ls[q];
        pl->leaf_len[q] = ll[q];
    }
    for (int q = 0; q < pl->nops; ++q) {
        pl->op_a[q] = slot(oa[q]);
        pl->op_b[q] = slot(ob[q]);
    }
    pl->root = slot(root);
    return 0;
}

// timing events come from a per-session pool (created on first use, reused
// once collect_timing has read them)
static hipError_t take_event(Session *s, hipEvent_t *e)
{
    if (s->enext == s->epool.size()) {
        hipEvent_t n = nullptr;
        const hipError_t rc = hipEventCreate(&n);
        if (rc != hipSuccess) return rc;
        s->epool.push_back(n);
    }
    *e = s->epool[s->enext++];
    return hipSuccess;
}

// Wait for an event by polling it (the blocking wait's wake-up cost ~0.1 ms
// per iteration boundary on the MI355X hosts): a busy poll for the first
// 200 us (the common case: the GPU is a few kernels behind), then polls with
// sched_yield between them, so a long wait does not hold a host core; after
// the session's sync timeout (IC_OPT_SYNC_TIMEOUT_MS, default 600 s) it gives
// up with hipErrorLaunchTimeOut and marks the session failed, so a kernel
// that never finishes fails the run instead of hanging its caller, and no
// later call reuses buffers its kernels may still be using.
static const auto kBusyPoll = std::chrono::microseconds(200);
static hipError_t poll_event(Session *s, hipEvent_t ev)
{
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    const auto spin = kBusyPoll;
    const auto limit = std::chrono::duration<double>(s->sync_timeout_s);
    hipError_t e;
    unsigned n = 0;
    while ((e = hipEventQuery(ev)) == hipErrorNotReady) {
        const auto dt = clk::now() - t0;
        if (dt > limit) {
            s->failed = true;
            return hipErrorLaunchTimeOut;
        }
        if (dt > spin) {
            sched_yield();
            // a peer lost by the transport (RCCL's asynchronous error): the
            // kernels queued behind its collective may never run
            if (s->comm && (++n & 255) == 0 && s->comm->remote_error()) {
                s->failed = true;
                s->comm_lost = true;
                return hipErrorLaunchTimeOut;
            }
        }
    }
    return e;
}

// Wait for a round's survivor count, which k_fit_state's last block publishes
// into host-mapped memory (a system-scope release store): the same polling as
// poll_event, on the value itself, so the round needs no event (a marker packet
// between the state kernel and the next sweep costs ~7 us per round boundary)
static hipError_t poll_count(Session *s, const int32_t *cnt)
{
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    const auto spin = kBusyPoll;
    const auto limit = std::chrono::duration<double>(s->sync_timeout_s);
    unsigned n = 0;
    while (__atomic_load_n(cnt, __ATOMIC_ACQUIRE) < 0) {
        const auto dt = clk::now() - t0;
        if (dt > limit) {
            s->failed = true;
            return hipErrorLaunchTimeOut;
        }
        if (dt > spin) {
            sched_yield();
            if (s->comm && (++n & 255) == 0 && s->comm->remote_error()) {
                s->failed = true;
                s->comm_lost = true;
                return hipErrorLaunchTimeOut;
            }
        }
    }
    return hipSuccess;
}

static hipError_t spin_sync(Session *s)
{
    hipError_t e = hipEventRecord(s->sev, s->stream);
    if (e != hipSuccess) return e;
    return poll_event(s, s->sev);
}

// Timed launches go through the dispatch packet (g_timing, ic_internal.h):
// no marker packets around them.  A wrapper that launched nothing drops its
// events; one that launched several kernels ends the interval with a marker.
#define LAUNCH(S, KID, CALL) LAUNCH_ON(S, KID, (S)->stream, CALL)
#define LAUNCH_ON(S, KID, ST, CALL)                                            \
    do {                                                                       \
        Timed t_{KID, nullptr, nullptr};                                       \
        const bool tm_ = (S)->timing && ((S)->timing_only < 0 || (S)->timing_only == (KID)); \
        if (tm_) {                                                             \
            CK(take_event((S), &t_.a));                                        \
            CK(take_event((S), &t_.b));                                        \
            g_timing = PendingTiming{t_.a, t_.b, 0, 0};                        \
        }                                                                      \
        const hipError_t lc_ = (CALL);                                         \
        const PendingTiming pt_ = g_timing;                                    \
        g_timing = PendingTiming{};                                            \
        CK(lc_);                                                               \
        if (tm_ && pt_.used) {                                                 \
            if (pt_.extra) CK(hipEventRecord(t_.b, (ST)));                     \
            (S)->events.push_back(t_);                                         \
        } else if (tm_) {                                                      \
            (S)->enext -= 2;   /* nothing launched: the pair goes back */      \
        }                                                                      \
    } while (0)

// exp(-2 pi i num / den), rounded from long double
double2 unit_root(long double num, long double den)
{
    const long double a = -2.0L * 3.141592653589793238462643383279502884L * num / den;
    return make_double2((double)cosl(a), (double)sinl(a));
}

// the DFT twiddles [nbin] exp(-2 pi i q / nbin)
std::vector<double2> host_twiddles(int nbin)
{
    std::vector<double2> tw(nbin);
    for (int q = 0; q < nbin; ++q) tw[q] = unit_root((long double)q, (long double)nbin);
    return tw;
}

// Twiddles of k_diag_p2 for nbin = N = 2^k: [M = N/2] exp(-2 pi i q/N) for the
// real-FFT post-processing, then for every Stockham stage after the first (radix
// R = 8 while >= 3 levels remain, then 4 or 2; Ns = product of earlier radices)
// the table w^(r k), w = exp(-2 pi i/(R Ns)), k < Ns, r = 1..R-1, as [k][r-1].
// Total <= N entries.
std::vector<double2> p2_twiddles(int N)
{
    std::vector<double2> t;
    if (N < 4 || (N & (N - 1))) return t;
    const int M = N / 2;
    for (int q = 0; q < M; ++q) t.push_back(unit_root(q, N));
    int lg = 0;
    while ((1 << lg) < M) ++lg;
    for (int done = 0, Ns = 1; done < lg;) {
        const int rem = lg - done, R = rem >= 3 ? 8 : (rem == 2 ? 4 : 2);
        if (Ns > 1)
            for (int k = 0; k < Ns; ++k)
                for (int r = 1; r < R; ++r) t.push_back(unit_root((long double)r * k, (long double)R * Ns));
        Ns *= R;
        done += R == 8 ? 3 : (R == 4 ? 2 : 1);
    }
    return t;
}

// FFT_L of v (L a power of two) in f64: the rotation's Stockham stages in
// their written order (phase_rotation.py _stockham with n = L, _dft8 / _dft4 in
// f64; radix 8 while three or more levels remain, then 4 or 2), tw =
// host_twiddles(L).  Host code under -ffp-contract=off: every operation one
// IEEE f64 operation, so numpy's czt_filter gives the same bits.
void stockham64(std::vector<double2> &v, const std::vector<double2> &tw)
{
    const int L = (int)v.size();
    std::vector<double2> o(L);
    const auto add = [](double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); };
    const auto sub = [](double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); };
    const auto dft4 = [&](double2 *b) {
        const double2 c0 = add(b[0], b[2]), c1 = sub(b[0], b[2]), c2 = add(b[1], b[3]), d = sub(b[1], b[3]);
        const double2 c3 = make_double2(d.y, -d.x);   // -i d
        b[0] = add(c0, c2);
        b[1] = add(c1, c3);
        b[2] = sub(c0, c2);
        b[3] = sub(c1, c3);
    };
    int lg = 0;
    while ((1 << lg) < L) ++lg;
    for (int ns = 1; lg > 0;) {
        const int R = lg >= 3 ? 8 : (1 << lg), G = L / R, step = L / (R * ns);
        for (int j = 0; j < G; ++j) {
            const int k = j % ns;
            double2 u[8];
            for (int q = 0; q < R; ++q) u[q] = v[j + q * G];
            if (ns > 1)
                for (int q = 1; q < R; ++q) {
                    const double2 w = tw[(size_t)q * k * step], x = u[q];
                    u[q] = make_double2(x.x * w.x - x.y * w.y, x.x * w.y + x.y * w.x);
                }
            if (R == 8) {
                const double s8 = 0.7071067811865476;
                double2 c[8];
                for (int q = 0; q < 4; ++q) {
                    c[q] = add(u[q], u[q + 4]);
                    c[q + 4] = sub(u[q], u[q + 4]);
                }
                c[5] = make_double2((c[5].x + c[5].y) * s8, (c[5].y - c[5].x) * s8);
                c[6] = make_double2(c[6].y, -c[6].x);
                c[7] = make_double2((c[7].y - c[7].x) * s8, -((c[7].x + c[7].y) * s8));
                dft4(c);
                dft4(c + 4);
                for (int q = 0; q < 4; ++q) {
                    u[2 * q] = c[q];
                    u[2 * q + 1] = c[q + 4];
                }
            } else if (R == 4) {
                dft4(u);
            } else {
                const double2 x = u[0], y = u[1];
                u[0] = add(x, y);
                u[1] = sub(x, y);
            }
            for (int q = 0; q < R; ++q) o[(size_t)(j - k) * R + k + (size_t)q * ns] = u[q];
        }
        v.swap(o);
        ns *= R;
        lg -= R == 8 ? 3 : (R == 4 ? 2 : 1);
    }
}

// The chirp-z rotation's per-length tables (RotateArgs.czt; phase_rotation.py
// czt_chirp / czt_filter), f32 pairs: [L] tw = exp(-2 pi i q / L), [L] the
// filter B = FFT_L(b) with b[j] = b[L - j] = conj(w[j]), j < n, built in f64 and
// rounded once, [n] the chirp w[j] = exp(-i pi (j^2 mod 2n) / n)
std::vector<float> czt_tables(int n)
{
    const int L = czt_length(n);
    const std::vector<double2> tw = host_twiddles(L);
    std::vector<double2> w(n), b(L, make_double2(0.0, 0.0));
    for (int j = 0; j < n; ++j) {
        w[j] = unit_root((long double)(((long long)j * j) % (2 * n)), (long double)(2 * n));
        b[j] = b[(L - j) % L] = make_double2(w[j].x, -w[j].y);
    }
    stockham64(b, tw);
    std::vector<float> t;
    t.reserve(czt_table_floats(n));
    const auto put = [&t](const std::vector<double2> &src) {
        for (const double2 &e : src) {
            t.push_back((float)e.x);
            t.push_back((float)e.y);
        }
    };
    put(tw);
    put(b);
    put(w);
    return t;
}

// k_diag_czt's per-length tables (DiagArgs.czt; diag_czt.py chirp / filter),
// f64 pairs: [L] tw = exp(-2 pi i q / L), [L] the filter B / L with B = FFT_L(b),
// b[j] = b[L - j] = conj(w[j]), j < m (the scale is a power of two: exact), [m]
// the chirp w[j] = exp(-i pi (j^2 mod 2m) / m); m = diag_czt_points(n), L =
// diag_czt_length(n)
std::vector<double2> diag_czt_tables(int n)
{
    const int m = diag_czt_points(n), L = diag_czt_length(n);
    std::vector<double2> t = host_twiddles(L), w(m), b(L, make_double2(0.0, 0.0));
    for (int j = 0; j < m; ++j) {
        w[j] = unit_root((long double)(((long long)j * j) % (2 * m)), (long double)(2 * m));
        b[j] = b[(L - j) % L] = make_double2(w[j].x, -w[j].y);
    }
    stockham64(b, t);
    const double sc = 1.0 / (double)L;
    for (double2 &e : b) e = make_double2(e.x * sc, e.y * sc);
    t.reserve(diag_czt_table_entries(n));
    t.insert(t.end(), b.begin(), b.end());
    t.insert(t.end(), w.begin(), w.end());
    return t;
}

int collect_timing(Session *s)
{
    if (s->events.empty()) return 0;
    CK(hipStreamSynchronize(s->stream));
    for (auto &e : s->events) {
        float ms = 0.f;
        CK(hipEventElapsedTime(&ms, e.a, e.b));
        s->kms[e.kid] += ms;
        s->klaunch[e.kid] += 1;
    }
    s->events.clear();
    s->enext = 0;
    return 0;
}

void free_all(Session *s)
{
    // hazard (d): a residual download may still be writing the caller's arrays
    // from res_q / res_so; it ends before the staging is freed
    if (s->dl_stream) {
        (void)hipStreamSynchronize(s->dl_stream);
        (void)hipStreamDestroy(s->dl_stream);
    }
    if (s->copy_stream) (void)hipStreamDestroy(s->copy_stream);
    if (s->dstream) (void)hipStreamDestroy(s->dstream);
    for (hipEvent_t ev : {s->slot_ev[0], s->slot_ev[1], s->fork_ev, s->join_ev, s->fork2_ev, s->enc_ev, s->dl_ev})
        if (ev) (void)hipEventDestroy(ev);
    s->mem.free_all();
    if (s->comm) {   // the transport's buffers
        void *xbufs[] = {s->xw_send, s->xw_recv, s->xf_send, s->xf_recv, s->xwg_send, s->xwg_recv, s->xfg_send,
                         s->xfg_recv, s->xd_send, s->xd_recv, s->xr_send, s->xr_recv, s->xt_send, s->xt_recv,
                         s->counters};
        for (void *b : xbufs)
            if (b) s->comm->release(b);
        s->counters = nullptr;
        delete s->comm;
        s->comm = nullptr;
    }
    if (s->h_rcount) (void)hipHostFree(s->h_rcount);
    if (s->h_small) (void)hipHostFree(s->h_small);
    if (s->sev) (void)hipEventDestroy(s->sev);
    for (auto &e : s->epool) (void)hipEventDestroy(e);
    s->epool.clear();
    s->events.clear();
    if (s->stream) (void)hipStreamDestroy(s->stream);
}

#define CM(S, call, what)                                                                         \
    do {                                                                                          \
        Timed t_{K_EXCHANGE, nullptr, nullptr};                                                   \
        const bool tm_ = (S)->timing && ((S)->timing_only < 0 || (S)->timing_only == K_EXCHANGE); \
        if (tm_) {                                                                                \
            CK(take_event((S), &t_.a));                                                           \
            CK(take_event((S), &t_.b));                                                           \
            CK(hipEventRecord(t_.a, (S)->stream));                                                \
        }                                                                                         \
        const int rc_ = (call);                                                                   \
        if (tm_) {                                                                                \
            CK(hipEventRecord(t_.b, (S)->stream));                                                \
            (S)->events.push_back(t_);                                                            \
        }                                                                                         \
        if (rc_ != 0) {                                                                           \
            (S)->comm->abort();                                                                   \
            return fail(IC_ECOMM, "shard %d/%d: %s exchange failed (%d)", (S)->rank, (S)->world,  \
                        what, rc_);                                                               \
        }                                                                                         \
    } while (0)

// Halving-tree plan (archive.py sb_tree) as a post-order stack program.
void sb_plan_rec(int lo, int hi, uint8_t *merges)
{
    if (hi - lo == 1) return;
    const int mid = lo + (hi - lo) / 2;
    sb_plan_rec(lo, mid, merges);
    sb_plan_rec(mid, hi, merges);
    merges[hi - 1]++;
}

SbPlan make_sb_plan(int n)
{
    SbPlan pl;
    memset(&pl, 0, sizeof pl);
    pl.n = n;
    if (n >= 1 && n <= kMaxSbLeaves) sb_plan_rec(0, n, pl.merges);
    return pl;
}

// shards.py channel_shards / row_owners; 0 or an error message
const char *shard_layout(int nsub, int nchan, int world, int32_t *chan0, int32_t *row0)
{
    if (world < 1 || (world & (world - 1))) return "world size must be a power of two";
    if (world > kMaxShards) return "world size too large";
    const int nsb = super_blocks(nchan);
    if (nsb < world) return "fewer 256-channel super-blocks than shards";
    int depth = 0;
    while ((1 << depth) < world) ++depth;
    for (int r = 0; r < world; ++r) {
        int lo = 0, hi = nsb;
        for (int d = depth - 1; d >= 0; --d) {
            const int mid = lo + (hi - lo) / 2;
            if ((r >> d) & 1)
                lo = mid;
            else
                hi = mid;
        }
        chan0[2 * r] = lo * kSuperBlock;
        chan0[2 * r + 1] = std::min(hi * kSuperBlock, nchan);
        row0[2 * r] = (int)((long)r * nsub / world);
        row0[2 * r + 1] = (int)((long)(r + 1) * nsub / world);
    }
    return nullptr;
}

// Window stage: per-subint window from the W-weighted total of `part`
// (unsharded: combine the super-blocks).  Sharded: reduce the local
// super-blocks to this shard's root, send each subint's root row to the rank
// that owns the row (all-to-all), the owner combines the world's roots in
// canonical order and searches the window, and the owners' windows are
// all-gathered (4 B per subint) - each root crosses the fabric once.
int window_stage(Session *s, int32_t *flags)
{
    const int nsub = s->p.nsub, nbin = s->p.nbin;
    if (!s->comm) {
        LAUNCH(s, K_WINDOW, launch_window(s->stream, s->part, (long)s->nsb * nbin, nbin, s->plan_sb, nsub, nbin,
                                          s->width, s->win, flags));
        return 0;
    }
    LAUNCH(s, K_SB_TREE, launch_sb_tree(s->stream, s->part, nullptr, s->plan_sb, nsub, nbin, nbin, s->xw_send));
    CM(s, s->comm->alltoallv(s->xw_send, s->wsb.data(), s->xw_recv, s->wrb.data(), s->stream), "window roots");
    if (s->rows_own > 0)
        LAUNCH(s, K_WINDOW, launch_window(s->stream, s->xw_recv, nbin, (long)s->rows_own * nbin, s->plan_top,
                                          s->rows_own, nbin, s->width, s->xwg_send, nullptr));
    CM(s, s->comm->allgather(s->xwg_send, s->xwg_recv, sizeof(int32_t) * s->wg_blk, s->stream), "windows");
    LAUNCH(s, K_SHARD_PACK, launch_unpack_windows(s->stream, s->geom, s->wg_blk, s->xwg_recv, s->win, flags));
    return 0;
}

// fscrunch + tscrunch from part2/wpart (sharded as window_stage: root rows of
// nbin + 1 doubles to the row owners, owners' F rows + wf all-gathered)
int scrunch_stage(Session *s)
{
    const int nsub = s->p.nsub, nbin = s->p.nbin;
    if (!s->comm) {
        LAUNCH(s, K_FSCRUNCH, launch_fscrunch(s->stream, s->part2, (long)s->nsb * nbin, nbin, s->wpart, s->nsb, 1,
                                              s->plan_sb, nsub, nbin, s->F, s->wf));
    } else {
        const long row = nbin + 1, own = (long)s->rows_own * row;
        LAUNCH(s, K_SB_TREE, launch_sb_tree(s->stream, s->part2, s->wpart, s->plan_sb, nsub, nbin, row, s->xf_send));
        CM(s, s->comm->alltoallv(s->xf_send, s->fsb.data(), s->xf_recv, s->frb.data(), s->stream), "fscrunch roots");
        if (s->rows_own > 0)
            LAUNCH(s, K_FSCRUNCH, launch_fscrunch(s->stream, s->xf_recv, row, own, s->xf_recv + nbin, row, own,
                                                  s->plan_top, s->rows_own, nbin, s->xfg_send,
                                                  s->xfg_send + (size_t)s->rows_pad * nbin));
        CM(s, s->comm->allgather(s->xfg_send, s->xfg_recv, sizeof(float) * s->fg_blk, s->stream), "fscrunch rows");
        LAUNCH(s, K_SHARD_PACK, launch_unpack_fscrunch(s->stream, s->geom, s->rows_pad, s->fg_blk, nbin, s->xfg_recv,
                                                       s->F, s->wf));
    }
    LAUNCH(s, K_TSCRUNCH, launch_tscrunch(s->stream, s->F, s->wf, nsub, nbin, s->T, s->T64, s->T2));
    return 0;
}

// phasor table f32(ic_phasor(k, delay[c], nbin)), k <= nbin/2, as f32 pairs
// (phase_rotation.py phasors; oracle orc_phasors; the rotation computes in
// f32): the same function the per-profile kernel evaluates on the device and
// rounds, so a table row and a profile with that delay agree
std::vector<float> make_phasors(int nbin, int nchan, const double *delay)
{
    const int m = nbin / 2;
    std::vector<float> ph(2 * (size_t)nchan * (m + 1));
    for (int c = 0; c < nchan; ++c)
        for (int k = 0; k <= m; ++k) {
            const double2 v = ic_phasor(k, delay[c], nbin);
            ph[2 * ((size_t)c * (m + 1) + k)] = (float)v.x;
            ph[2 * ((size_t)c * (m + 1) + k) + 1] = (float)v.y;
        }
    return ph;
}

RotateArgs rotate_args(Session *s, const float *in, const float *base, int sign, const int32_t *flags, float *out,
                       long ldo)
{
    RotateArgs a{};
    a.in = in;
    a.ld_in = s->p.nbin;
    a.base = base;
    a.ph = s->ph;
    a.delay2 = s->delay2;
    // an archive stored dedispersed: its dedisperse is a no-op (archive.py),
    // only the residual's dededisperse rotates
    a.identity = sign > 0 && s->p.input_dedispersed;
    a.sign = sign;
    a.tw = s->tw;
    a.tw_p2 = s->tw_p2;
    a.czt = s->czt;
    a.flags = flags;
    a.nsub = s->p.nsub;
    a.nchan = s->nchan;
    a.nbin = s->p.nbin;
    a.out = out;
    a.ldo = ldo;
    a.grid_cap = s->grid_cap;
    return a;
}

// the iteration's residual rows f32(a T - D) (remove_profile1d, ic.py:277-288),
// rotated back to the dispersed frame (dededisperse, ic.py:104) -> s->R
RotateArgs residual_rotate_args(Session *s, int pr_start, int pr_end)
{
    RotateArgs a = rotate_args(s, s->D, nullptr, -1, nullptr, s->R, s->p.nbin);
    a.ld_in = s->ldD;
    a.T64 = s->T64;
    a.amp = s->amp;
    a.info = s->info;
    a.pr_on = s->p.pr_on;
    a.pr_factor = s->p.pr_factor;
    a.pr_start = pr_start;
    a.pr_end = pr_end;
    a.in_tiled = s->dtiled;
    return a;
}

// the FFT mode's residual rotation also computes comprehensive_stats of its rows
// (no R, no DIAG_STATS pass): when the option is on and the kernel serves nbin
bool rot_stats_on(const Session *s)
{
    return s->fftded && s->rot_stats && rotate_stats_supported(s->p.nbin, s->p.data_f64 != 0);
}
void with_stats(Session *s, RotateArgs &a)
{
    a.out = nullptr;
    a.w0 = s->w0;
    a.tw_p2 = s->tw_p2;
    a.std_o = s->std_;
    a.mean_o = s->mean;
    a.ptp_o = s->ptp;
    a.fft_o = s->fft;
}

// fit-cube preparation (iterative_cleaner.py:96-100): baseline with w0, dedisperse.
// The w0 baseline (window + per-profile levels) is also the template stage's
// baseline of the first iteration (W == w0).  A shard also hands the validity
// of its profiles to the row owners (static for the whole run).
int prepare(Session *s)
{
    const int nsub = s->p.nsub, nchan = s->nchan, nbin = s->p.nbin;
    CK(launch_valid(s->stream, s->w0, s->valid, s->W, s->hist, s->P));
    if (s->comm) {
        LAUNCH(s, K_SHARD_PACK,
               launch_pack_rows(s->stream, s->geom, nchan, nullptr, nullptr, nullptr, nullptr, s->valid, s->xd_send,
                                s->grid_cap));
        CM(s, s->comm->alltoallv(s->xd_send, s->vsb.data(), s->xd_recv, s->vrb.data(), s->stream), "valid rows");
        LAUNCH(s, K_SHARD_PACK,
               launch_assemble_rows(s->stream, s->geom, s->xd_recv, nullptr, nullptr, nullptr, nullptr, s->valid_r,
                                    s->grid_cap));
    }
    if (s->fftded) {
        // remove_baseline reads the dedispersed view rot(raw) (archive.py
        // _ded_view); dedisperse then rotates the data it leaves, f32(raw - base0):
        // that is the fit cube D and iteration 1's template rows Tc (W == w0)
        LAUNCH(s, K_ROTATE, launch_rotate(s->stream, rotate_args(s, s->raw, nullptr, +1, nullptr, s->dr, nbin)));
        LAUNCH(s, K_CHAN_PARTIALS,
               launch_chan_partials(s->stream, 0, s->dr, s->w0, s->zshift, nullptr, nullptr, nsub, nchan, nbin,
                                    s->part, nullptr, nullptr, nullptr, 0, 0, s->exA, nullptr));
        if (int rc = window_stage(s, nullptr)) return rc;
        LAUNCH(s, K_BASE,
               launch_base(s->stream, s->dr, s->zshift, s->win, nullptr, nsub, nchan, nbin, s->width, s->base0,
                           s->grid_cap));
        RotateArgs ra = rotate_args(s, s->raw, s->base0, +1, nullptr, s->Tc, nbin);
        ra.out2 = s->D;
        ra.ldo2 = s->ldD;
        ra.out2_tiled = s->dtiled;
        LAUNCH(s, K_ROTATE, launch_rotate(s->stream, ra));
        CK(hipMemcpyAsync(s->base, s->base0, sizeof(float) * s->P, hipMemcpyDeviceToDevice, s->stream));
        CK(hipMemsetAsync(s->wflag + nsub, 0, sizeof(int32_t), s->stream));
        return 0;
    }
    LAUNCH(s, K_CHAN_PARTIALS,
           launch_chan_partials(s->stream, 0, s->raw, s->w0, s->shift, nullptr, nullptr, nsub, nchan, nbin, s->part,
                                nullptr, nullptr, nullptr, 0, 0, s->exA, nullptr));
    if (int rc = window_stage(s, nullptr)) return rc;
    LAUNCH(s, K_BASE,
           launch_base(s->stream, s->raw, s->shift, s->win, nullptr, nsub, nchan, nbin, s->width, s->base0,
                       s->grid_cap));
    // the fit cube D = f32(ded - base0) is written by iteration 1's template
    // pass (chan_partials mode 3), which reads the same values
    CK(hipMemcpyAsync(s->base, s->base0, sizeof(float) * s->P, hipMemcpyDeviceToDevice, s->stream));
    CK(hipMemsetAsync(s->wflag + nsub, 0, sizeof(int32_t), s->stream));
    return 0;
}

// Template of iteration `iter` (iterative_cleaner.py:88-94): remove_baseline
// with the current weights W, dedisperse, fscrunch, tscrunch.  The baseline
// level of a profile depends on W only through its subint's window (the window
// position is the argmin over the W-weighted total; the level is the raw
// window mean), so s->base/s->win carry over between iterations: one read of
// the cube computes the W-weighted total AND the fscrunch partials with the
// carried baseline; subints whose window moved get their levels and partials
// recomputed (flagged launches that are empty when nothing moved).
int iteration_template(Session *s, int iter)
{
    const int nsub = s->p.nsub, nchan = s->nchan, nbin = s->p.nbin;
    if (s->fftded) {
        // FFT dedispersion: the window totals and levels read rot(raw); the rows
        // rot(f32(raw - base)) of subints whose window moved are re-rotated, and
        // the fscrunch partials are taken over those rows (no shift, no level).
        // Incremental (IC_OPT_TEMPLATE_INCR): both sums move through the changed
        // channels (k_chan_delta, part from rot(raw), part2 from the rows), the
        // subints whose window moved are summed again after their re-rotation.
        const bool incr = iter > 1 && s->incr;
        if (iter > 1) {
            if (incr) {
                const float *Wo = s->hist + (size_t)(iter - 2) * s->P;
                LAUNCH(s, K_CHAN_PARTIALS,
                       launch_chan_delta(s->stream, s->dr, s->zshift, s->zbase, s->W, Wo, nsub, nchan, nbin, s->part,
                                         s->part2, s->wpart, s->exA, s->exF, s->Tc));
            } else {
                LAUNCH(s, K_CHAN_PARTIALS,
                       launch_chan_partials(s->stream, 0, s->dr, s->W, s->zshift, nullptr, nullptr, nsub, nchan, nbin,
                                            s->part, nullptr, nullptr, nullptr, 0, 0, s->exA, nullptr));
            }
            if (int rc = window_stage(s, s->wflag)) return rc;
            LAUNCH(s, K_BASE,
                   launch_base(s->stream, s->dr, s->zshift, s->win, s->wflag, nsub, nchan, nbin, s->width, s->base,
                               s->grid_cap));
            LAUNCH(s, K_ROTATE,
                   launch_rotate(s->stream, rotate_args(s, s->raw, s->base, +1, s->wflag, s->Tc, nbin)));
        }
        LAUNCH(s, K_CHAN_PARTIALS,
               launch_chan_partials(s->stream, 1, s->Tc, s->W, s->zshift, s->zbase, incr ? s->wflag : nullptr, nsub,
                                    nchan, nbin, nullptr, s->part2, s->wpart, nullptr, 0, 0, nullptr, s->exF));
        return scrunch_stage(s);
    }
    if (iter == 1) {   // W == w0: the carried baseline is exactly prepare()'s; also writes D (exact fit)
        LAUNCH(s, K_CHAN_PARTIALS,
               launch_chan_partials(s->stream, s->D ? 3 : 1, s->raw, s->W, s->shift, s->base, nullptr, nsub, nchan,
                                    nbin, nullptr, s->part2, s->wpart, s->D, s->ldD, s->dtiled, nullptr, s->exF));
    } else {
        if (s->incr) {
            // the sums of the previous iteration moved through the changed channels
            const float *Wo = s->hist + (size_t)(iter - 2) * s->P;
            LAUNCH(s, K_CHAN_PARTIALS,
                   launch_chan_delta(s->stream, s->raw, s->shift, s->base, s->W, Wo, nsub, nchan, nbin, s->part,
                                     s->part2, s->wpart, s->exA, s->exF));
        } else {
            LAUNCH(s, K_CHAN_PARTIALS,
                   launch_chan_partials(s->stream, 2, s->raw, s->W, s->shift, s->base, nullptr, nsub, nchan, nbin,
                                        s->part, s->part2, s->wpart));
        }
        if (int rc = window_stage(s, s->wflag)) return rc;
        LAUNCH(s, K_BASE,
               launch_base(s->stream, s->raw, s->shift, s->win, s->wflag, nsub, nchan, nbin, s->width, s->base,
                           s->grid_cap));
        LAUNCH(s, K_CHAN_PARTIALS,
               launch_chan_partials(s->stream, 1, s->raw, s->W, s->shift, s->base, s->wflag, nsub, nchan, nbin,
                                    nullptr, s->part2, s->wpart, nullptr, 0, 0, nullptr, s->exF));
    }
    return scrunch_stage(s);
}

// The rules of std_template.py check(): 0 or the message
const char *std_check(const float *S, int nbin)
{
    if (nbin < 4) return "fewer than 4 bins";
    bool constant = true;
    for (int i = 0; i < nbin; ++i) {
        if (!std::isfinite(S[i])) return "a non-finite value";
        if (S[i] != S[0]) constant = false;
    }
    return constant ? "a constant profile" : nullptr;
}

// m of std_template.py ccf(): the sum of f64(S) in ascending index, over nbin
// (host code under -ffp-contract=off: one IEEE addition per sample)
double std_mean_of(const float *S, int nbin)
{
    double acc = 0.0;
    for (int i = 0; i < nbin; ++i) acc = acc + (double)S[i];
    return acc / (double)nbin;
}

// the one-profile rotation of the `frac` alignment: S by -shift, the delay read
// from the record on the device (k_rotate's per-profile-delay path)
RotateArgs std_rotate_args(const float *S, const StdAlignRec *rec, int nbin, const double2 *tw, const double2 *tw_p2,
                           float *out, int grid_cap)
{
    RotateArgs a{};
    a.in = S;
    a.ld_in = nbin;
    a.delay2 = &rec->shift;
    a.sign = -1;
    a.tw = tw;
    a.tw_p2 = tw_p2;
    a.nsub = 1;
    a.nchan = 1;
    a.nbin = nbin;
    a.out = out;
    a.ldo = nbin;
    a.grid_cap = grid_cap;
    return a;
}

// The standard template (ic_set_std_template) takes the place of iteration 1's
// own: s->T holds A, the archive's first template (iteration_template(s, 1));
// the standard is aligned against it and installed as T, T64 and T2, all on the
// session's stream with no host read (std_template.py; DESIGN.md "Standard
// template").  On a shard every rank holds the same A after scrunch_stage and
// aligns for itself: the same bits on every rank, no exchange.
int std_stage(Session *s)
{
    const int nbin = s->p.nbin;
    if (s->std_mode == IC_ALIGN_NONE) {
        CK(hipMemsetAsync(s->std_rec, 0, sizeof(StdAlignRec), s->stream));
    } else {
        LAUNCH(s, K_STD_ALIGN,
               launch_std_ccf(s->stream, s->std_S, s->T, nbin, s->std_mean, s->std_c, s->grid_cap));
        LAUNCH(s, K_STD_ALIGN, launch_std_peak(s->stream, s->std_c, nbin, s->std_rec));
    }
    if (s->std_mode == IC_ALIGN_FRAC)
        LAUNCH(s, K_ROTATE, launch_rotate(s->stream, std_rotate_args(s->std_S, s->std_rec, nbin, s->tw, s->tw_p2,
                                                                     s->std_rot, s->grid_cap)));
    LAUNCH(s, K_STD_INSTALL,
           launch_std_install(s->stream, s->std_S, s->std_rot, s->std_rec, s->std_mode, nbin, s->ldD, s->T, s->T64,
                              s->T2, s->grid_cap));
    return 0;
}

// Row medians/MADs of a shard: the diagnostics rows go to their owners
// (all-to-all), each owner runs the row selections over whole rows, and the
// results are all-gathered into row_med/row_mad [4][nsub].
// its first half, shared with shard_rowtrends: the rows to their owners
int shard_rows_to_owners(Session *s)
{
    LAUNCH(s, K_SHARD_PACK,
           launch_pack_rows(s->stream, s->geom, s->nchan, s->std_, s->mean, s->fft, s->ptp, nullptr, s->xd_send,
                            s->grid_cap));
    CM(s, s->comm->alltoallv(s->xd_send, s->dsb.data(), s->xd_recv, s->drb.data(), s->stream), "diagnostics rows");
    LAUNCH(s, K_SHARD_PACK,
           launch_assemble_rows(s->stream, s->geom, s->xd_recv, s->std_r, s->mean_r, s->fft_r, s->ptp_r, nullptr,
                                s->grid_cap));
    return 0;
}
// the owner's whole rows as lines; med / MAD [4][rows_own] go to `slot`
LineStatsArgs owned_rows_args(Session *s, const LineStatsArgs &la, double *slot)
{
    LineStatsArgs lr;
    lr.nsub = s->rows_own;
    lr.nchan = s->geom.nchan_g;
    lr.valid = s->valid_r;
    lr.std_d = s->std_r;
    lr.mean_d = s->mean_r;
    lr.fft_d = s->fft_r;
    lr.ptp_d = s->ptp_r;
    lr.ptp_f32 = la.ptp_f32;
    lr.grp_waves = la.grp_waves;
    lr.grp_minlen = la.grp_minlen;
    lr.col_med = lr.col_mad = nullptr;
    lr.row_med = slot;
    lr.row_mad = slot + 4 * s->rows_own;
    return lr;
}
int shard_rowstats(Session *s, const LineStatsArgs &la)
{
    if (int rc = shard_rows_to_owners(s)) return rc;
    const LineStatsArgs lr = owned_rows_args(s, la, s->xr_send);
    LAUNCH(s, K_LINESTATS, launch_lines(s->stream, lr, nullptr, nullptr, 2));
    CM(s, s->comm->allgather(s->xr_send, s->xr_recv, sizeof(double) * 8 * s->rows_pad, s->stream), "row statistics");
    LAUNCH(s, K_SHARD_PACK, launch_unpack_rowstats(s->stream, s->geom, s->rows_pad, s->xr_recv, la.row_med, la.row_mad));
    return 0;
}

// The detrended sibling (ic_shard_enable_detrend): the same rows to the same
// owners; each owner fits its whole rows (length nchan_g, as one GPU would) and
// writes med, MAD and coefficients straight into its slot of xt_send (med
// [4][rows_own], mad [4][rows_own], TrendCoef [4][rows_own][ms]; ms = 1 when
// unpieced); one all-gather of the slots, scattered by row owner into la.row_med /
// la.row_mad [4][nsub] and ta.row_coef [4][nsub][ms][4].  pa == nullptr: whole
// lines.  A rank that owns no rows launches no fit and still joins the collective.
int shard_rowtrends(Session *s, const LineStatsArgs &la, const TrendArgs &ta, const PieceArgs *pa)
{
    if (int rc = shard_rows_to_owners(s)) return rc;
    const size_t ms = pa ? (size_t)pa->row_np : 1;
    const size_t slot = (size_t)s->rows_pad * (8 + 16 * ms);
    if (!s->xt_send || !s->xt_recv || s->xt_ms != ms) return fail(IC_ESTATE, "no exchange buffers for the row trends");
    if (s->rows_own > 0) {
        const LineStatsArgs lr = owned_rows_args(s, la, s->xt_send);
        TrendArgs tr = ta;
        tr.col_coef = nullptr;
        tr.row_coef = s->xt_send + 8 * (size_t)s->rows_own;
        LAUNCH(s, K_LINESTATS, launch_lines(s->stream, lr, &tr, pa, 2));
    }
    CM(s, s->comm->allgather(s->xt_send, s->xt_recv, sizeof(double) * slot, s->stream), "row trends");
    LAUNCH(s, K_SHARD_PACK,
           launch_unpack_rowtrends(s->stream, s->geom, s->rows_pad, (int)ms, s->xt_recv, la.row_med, la.row_mad,
                                   ta.row_coef, s->grid_cap));
    return 0;
}

// exact scipy leastsq for every profile (ic.py:266-272).
// Rounds of k_fit_pass + k_fit_state over a compacted list of the profiles
// that still need a data sweep.  Each round's survivor count lands in
// the low word of ctr[r] on the device; kernels read their list length there, so the
// host only needs an UPPER bound to size grids (counts never grow) and reads
// the counts one round behind: the stream always has the next round queued.
// Once the bound drops to tail_threshold (default kTailProfiles; 0 = never),
// k_fit_tail finishes the rest in one launch (one wave per profile).
// fork != nullptr: after round s->diag_fork the diagnostics of the profiles
// already fitted run on s->dstream (fork_diag); the survivors of that round
// are kept in the third list buffer for the main stream's second pass.
int fork_diag(Session *s, const DiagArgs &da, int r);
// after the round counters (and two spare words): the tail's sweep counter
// (u64, accumulating over a run: zeroed and read once per run by ic_run)
unsigned long long *tail_counter(Session *s) { return (unsigned long long *)(s->rcount + kRoundWords + 2); }

int run_fit(Session *s, const DiagArgs *fork)
{
    s->fork_round = -1;
    s->tail_split = false;
    const long P = (long)s->P;
    const int nbin = s->p.nbin;
    // zeroes too: per round, blocks done << 32 | survivors (the tail's sweep
    // counter after them accumulates over the run: zeroed and read once per
    // run by ic_run), and the late flags the fork round's state kernel sets
    CK(launch_fit_init(s->stream, s->fs, P, s->rcount, kRoundWords + 2, fork ? s->late : nullptr));
    CK(launch_fit_prep(s->stream, s->fs, s->T64, nbin));
    unsigned long long *ctr = (unsigned long long *)s->rcount;
    unsigned *done = (unsigned *)(s->rcount + 2 * kMaxRounds);
    unsigned long long *tail_sweeps = tail_counter(s);
    int32_t *bufs[3] = {s->lists, s->lists + P, s->lists + 2 * P};
    const int32_t *cur = nullptr;                    // round 0: all profiles
    const unsigned long long *cin = nullptr;         // the round's packed list counts (RoundList)
    long bound = P;                                 // >= the active count of the next round
    int rounds = 0;
    bool tail = false;
    int flagged = -1;   // the fork round, once its survivors are flagged and pass A not yet queued
    for (int r = 0;; ++r) {
        if (r >= kMaxRounds) return fail(IC_EHIP, "lmdif did not terminate after %d rounds", r);
        if (bound <= s->tail_threshold) {
            if (flagged >= 0) {
                if (int rc = fork_diag(s, *fork, flagged)) return rc;
                flagged = -1;
            }
            // (auto: profiles of >= 2048 bins, whose tail and statistics are long
            // enough to share the chip: C5 48.9-49.3 ms split against 50.7-50.8;
            // at 1024 bins the statistics' 8-wave blocks beside the tail stretch
            // its critical path, C2 26.0 against 25.5-25.6, C3 173.0 against
            // 171.7; C1 1.29-1.31 against 1.26-1.27; C4 2.91-2.93 against 2.94-2.96)
            const bool split = fork && (s->tail_split_mode == IC_TAIL_SPLIT_ON ||
                                        (s->tail_split_mode == IC_TAIL_SPLIT_AUTO && nbin >= 2048));
            if (split && s->fork_round >= 0 && cur && !s->fftded) {
                // the second fork: the fork round's survivors fitted by now (not in
                // the tail's list, marked here) are measured on dstream beside the tail
                CK(launch_mark_list(s->stream, cur, cin, P, bound, s->tmark, 1));
                CK(hipEventRecord(s->fork2_ev, s->stream));
                CK(hipStreamWaitEvent(s->dstream, s->fork2_ev, 0));
                DiagArgs b1 = *fork;
                b1.list = s->lists + 2 * P;
                b1.nctr = ctr + s->fork_round;
                b1.skip = s->tmark;
                LAUNCH_ON(s, K_DIAG, s->dstream, launch_diag(s->dstream, b1));
                CK(hipEventRecord(s->join_ev, s->dstream));
                s->tail_split = true;
                s->tail_list = cur;
                s->tail_cin = cin;
                s->tail_bound = bound;
            }
            LAUNCH(s, K_FIT_TAIL, launch_fit_tail(s->stream, s->D, s->T64, P, nbin, s->ldD, s->dtiled, cur, cin, bound,
                                                  s->fs, s->amp, s->info, tail_sweeps, s->grid_cap));
            tail = true;
            break;
        }
        const bool fork_here = fork && r == s->diag_fork;
        int32_t *next = fork_here ? bufs[2] : bufs[r & 1];
        LAUNCH(s, K_FIT_PASS, launch_fit_pass(s->stream, s->D, s->T64, P, nbin, s->ldD, s->dtiled, cur, cin, bound,
                                                s->fs, r == 0));
        __atomic_store_n(s->h_rcount + r, -1, __ATOMIC_RELAXED);
        LAUNCH(s, K_FIT_STATE, launch_fit_state(s->stream, s->fs, P, cur, cin, bound, s->amp, s->info, next,
                                                ctr + r, done + r, s->d_h_rcount + r, fork_here ? s->late : nullptr));
        if (fork_here) flagged = r;
        // pass A is queued fork_delay rounds after the flags: the first late
        // rounds are the largest and run alone
        if (flagged >= 0 && r >= flagged + s->fork_delay) {
            if (int rc = fork_diag(s, *fork, flagged)) return rc;
            flagged = -1;
        }
        ++rounds;
        cur = next;
        cin = ctr + r;   // packed A / B counts of the next round's list
        if (r >= 1) {
            // count after round r-1 (= input of round r) bounds the count after round r
            CK(poll_count(s, s->h_rcount + (r - 1)));
            const long c = s->h_rcount[r - 1];
            if (c == 0) break;   // round r had nothing to do
            bound = c;
        }
    }
    if (flagged >= 0)
        if (int rc = fork_diag(s, *fork, flagged)) return rc;
    // no stream synchronisation: the counts below were all read by the loop
    // (after the event of their round), so the diagnostics queue right behind
    // the last fit kernel
    int64_t swept = rounds > 0 ? P : 0;   // round 0 input
    for (int r = 0; r + 1 < rounds; ++r) swept += s->h_rcount[r];
    int effective = rounds;
    if (!tail) {
        // trailing rounds that had an empty input list
        while (effective > 1 && s->h_rcount[effective - 2] == 0) --effective;
    }
    s->fit_rounds = effective;
    s->stats.fit_rounds += effective;
    s->stats.fit_profile_sweeps += swept;
    return 0;
}

// The fork (run_fit, round r): the profiles that round r's state kernel did
// not flag in s->late have their final amp / info, so their diagnostics
// (pass A: k_diag_cl skipping the flagged ones) run on dstream, ordered after
// round r only, while the main stream goes on with the late rounds and the
// tail (latency-bound: a few thousand waves).  The flagged profiles, round r's
// survivor list in the third list buffer, get pass B on the main stream after
// the fit (run_impl), which then joins dstream.
int fork_diag(Session *s, const DiagArgs &da, int r)
{
    CK(hipEventRecord(s->fork_ev, s->stream));
    CK(hipStreamWaitEvent(s->dstream, s->fork_ev, 0));
    if (s->fftded) {   // their residual rows, rotated back (run_impl: the rest after the fit)
        RotateArgs ra = residual_rotate_args(s, s->pr_lo, s->pr_hi);
        ra.late = s->late;
        ra.late_sel = 0;
        if (rot_stats_on(s)) with_stats(s, ra);
        LAUNCH_ON(s, K_ROTATE, s->dstream, launch_rotate(s->dstream, ra));
    }
    if (!rot_stats_on(s)) {
        DiagArgs a = da;
        a.skip = s->late;
        LAUNCH_ON(s, K_DIAG, s->dstream, launch_diag(s->dstream, a));
    }
    CK(hipEventRecord(s->join_ev, s->dstream));
    s->fork_round = r;
    return 0;
}

}  // namespace

extern "C" {

int ic_abi_version(void) { return IC_ABI_VERSION; }

int ic_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *ic_last_error(void) { return g_err.c_str(); }

const char *ic_kernel_name(int kernel)
{
    if (kernel < 0 || kernel >= K_COUNT) return "";
    return kKernelNames[kernel];
}

}  // extern "C"

namespace {

// Shared by every create entry point.  sharded: this session is channel shard
// `rank` of `world` (world may be 1: the exchanges then run over a one-rank
// transport, which tests it end to end); make_comm() builds the transport
// after the device is current.
template <typename MakeComm>
int create_session(const ic_params *params, int device, int rank, int world, bool sharded, MakeComm make_comm,
                   void **out)
{
    if (!params || !out) return fail(IC_EINVAL, "null argument");
    *out = nullptr;
    const ic_params &p = *params;
    if (p.nsub <= 0 || p.nchan <= 0 || p.nbin <= 0)
        return fail(IC_EINVAL, "bad shape nsub=%d nchan=%d nbin=%d", p.nsub, p.nchan, p.nbin);
    if (p.nbin > 32768) return fail(IC_EINVAL, "nbin=%d > 32768 unsupported", p.nbin);
    if (p.nsub > 16384 || p.nchan > 16384)
        return fail(IC_EINVAL, "line length > 16384 unsupported (nsub=%d nchan=%d)", p.nsub, p.nchan);
    if (p.max_iter < 0) return fail(IC_EINVAL, "max_iter < 0");
    if (p.fit_mode != IC_FIT_EXACT && p.fit_mode != IC_FIT_CLOSED)
        return fail(IC_EINVAL, "fit_mode %d unsupported", p.fit_mode);
    if (p.dedisp_mode != IC_DEDISP_SHIFT && p.dedisp_mode != IC_DEDISP_FFT && p.dedisp_mode != IC_DEDISP_FFT_ANY)
        return fail(IC_EINVAL, "dedisp_mode %d unsupported", p.dedisp_mode);
    // IC_DEDISP_FFT_ANY (opt-in) is IC_DEDISP_FFT plus the chirp-z rotation of the other lengths in 16..4096
    const bool fft_any = p.dedisp_mode == IC_DEDISP_FFT_ANY, fft_mode = fft_any || p.dedisp_mode == IC_DEDISP_FFT;
    const bool czt = fft_any && czt_supported(p.nbin);
    if (p.input_dedispersed != 0 && (p.input_dedispersed != 1 || !fft_mode))
        return fail(IC_EINVAL, "input_dedispersed=%d needs dedisp_mode IC_DEDISP_FFT (0 or 1)", p.input_dedispersed);
    if (fft_mode && !rotate_supported(p.nbin) && !czt)
        return fail(IC_EINVAL, "fractional dedispersion needs " IC_ROT_NBIN_FMT IC_CZT_NBIN_FMT " (nbin=%d)",
                    IC_ROT_NBIN_ARGS, IC_CZT_NBIN_ARGS, p.nbin);
    // launch_diag has no DIAG_FIT at these lengths (k_diag_mr: EXACT, CLOSED and STATS)
    if (fft_mode && p.fit_mode == IC_FIT_CLOSED && mr_supported(p.nbin))
        return fail(IC_EINVAL,
                    "fit_mode IC_FIT_CLOSED with fractional dedispersion needs a power-of-two nbin in %d..%d; "
                    "a mixed-radix nbin takes IC_FIT_EXACT (nbin=%d)", kP2Min, kP2Max, p.nbin);
    if (czt && p.fit_mode == IC_FIT_CLOSED)
        return fail(IC_EINVAL,
                    "fit_mode IC_FIT_CLOSED with fractional dedispersion needs a power-of-two nbin in %d..%d; "
                    "a chirp-z nbin (IC_DEDISP_FFT_ANY) takes IC_FIT_EXACT (nbin=%d)", kP2Min, kP2Max, p.nbin);
    if (diag_lds_bytes(p.nbin) > kLdsBlockMax)
        return fail(IC_EINVAL, "nbin=%d needs %zu bytes of LDS for the diagnostics (> 160 KiB)", p.nbin,
                    diag_lds_bytes(p.nbin));
    if (window_lds_bytes(p.nbin) > kLdsBlockMax)
        return fail(IC_EINVAL, "nbin=%d needs %zu bytes of LDS for the baseline window (> 160 KiB)", p.nbin,
                    window_lds_bytes(p.nbin));
    if (world < 1 || rank < 0 || rank >= world) return fail(IC_EINVAL, "bad rank %d / world %d", rank, world);
    std::vector<int32_t> cr(2 * world), rr(2 * world);
    if (const char *e = shard_layout(p.nsub, p.nchan, world, cr.data(), rr.data()))
        return fail(IC_EINVAL, "cannot shard nchan=%d over %d: %s", p.nchan, world, e);
    if (int rc = select_device(device)) return rc;
    Session *s = new Session();
    s->p = p;
    s->device = device;
    s->rank = rank;
    s->world = world;
    s->c0 = cr[2 * rank];
    s->nchan = cr[2 * rank + 1] - cr[2 * rank];
    s->P = (size_t)p.nsub * s->nchan;
    s->N = s->P * (size_t)p.nbin;
    s->nsb = super_blocks(s->nchan);
    s->plan_sb = make_sb_plan(s->nsb);
    s->plan_top = make_sb_plan(world);
    s->geom.world = world;
    s->geom.rank = rank;
    s->geom.nsub = p.nsub;
    s->geom.nchan_g = p.nchan;
    for (int r = 0; r < world; ++r) {
        s->geom.chan0[r] = cr[2 * r];
        s->geom.row0[r] = rr[2 * r];
    }
    s->geom.chan0[world] = p.nchan;
    s->geom.row0[world] = p.nsub;
    s->rows_own = rr[2 * rank + 1] - rr[2 * rank];
    s->rows_pad = (p.nsub + world - 1) / world;
    s->ldD = ((p.nbin + kFitTile - 1) / kFitTile) * kFitTile;
    s->Ppad = ((s->P + 63) / 64) * 64;
    s->width = (int)(p.baseline_duty * (double)p.nbin);
    if (s->width < 1) s->width = 1;
    auto bail = [&](int code) {
        free_all(s);
        delete s;
        return code;
    };
#define AL(ptr, n)                                                                                    \
    do {                                                                                              \
        if (s->mem.alloc(&(ptr), (n)) != hipSuccess)                                                  \
            return bail(fail(IC_ENOMEM, "hipMalloc(%s, %zu elements) failed", #ptr, (size_t)(n)));    \
    } while (0)
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess)
        return bail(fail(IC_EHIP, "hipStreamCreate failed"));
    // the diagnostics fork's stream exists for every session it can serve
    // (IC_OPT_DIAG_FORK may switch it on or off before any run)
    if (p.fit_mode == IC_FIT_EXACT) {
        // (a higher priority for the fit's stream measured no different)
        if (hipStreamCreateWithFlags(&s->dstream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&s->fork_ev, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s->join_ev, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s->fork2_ev, hipEventDisableTiming) != hipSuccess)
            return bail(fail(IC_EHIP, "diagnostics stream / events failed"));
    }
    const size_t P = s->P, N = s->N;
    const int nsub = p.nsub, nchan = s->nchan, nbin = p.nbin;
    const bool exact = p.fit_mode == IC_FIT_EXACT;
    // the fit's lists hold int32 profile indices, its round counts are 32-bit fields (RoundList)
    if (exact && P >= (1ull << 31))
        return bail(fail(IC_EINVAL, "the exact fit takes < 2^31 profiles per session or shard (%zu)", P));
    AL(s->slot_raw[0], N);
    s->raw = s->slot_raw[0];
    // the closed-form fit reads the raw cube (no fit cube, no lmdif state), unless
    // the dedispersion is the FFT rotation: then the rotated fit cube is kept
    if (exact || fft_mode) {
        AL(s->D, s->Ppad * (size_t)s->ldD);
        if (hipMemset(s->D, 0, sizeof(float) * s->Ppad * (size_t)s->ldD) != hipSuccess)
            return bail(fail(IC_EHIP, "hipMemset(D) failed"));
    }
    AL(s->TT, 1);
    s->fftded = fft_mode;
    // The FFT mode forks too (round 6): its forked pass is the residual rotation
    // that measures the rows, one kernel since the statistics moved into it, and
    // it now hides behind the late fit rounds (C2 --dedisp fft 45.51-45.70 ->
    // 45.03-45.06 ms per clean, per-profile delays 47.23-47.44 -> 47.04-47.19,
    // alternating on one box; round 4, with two kernels per forked pass and the
    // radix-2 rotation, it had lost: 55.4-55.5 unforked, 56.7-56.9 forked)
    // large sessions hand over later: C2 (1.15 M profiles) 26.49-26.56 ms per
    // clean at 8192, 26.19-26.23 at 4096 (2048: 26.23-26.28, 6144: 26.30-26.34),
    // C3 flat; C4 and C5 lose at 4096 (2.90 -> 3.02-3.04, 46.5 -> 46.9)
    if (P >= ((size_t)1 << 20)) s->tail_threshold = kTailProfilesLarge;
    // long profiles hand over earlier: C5 (4096 bins) 46.1-47.0 ms at 8192,
    // 45.5-46.2 at 12288 (C4 at 512 bins flat from 6144 to 12288)
    else if (nbin >= 2048) s->tail_threshold = kTailProfilesLong;
    // long profiles take more rounds before their late phase: C5 (4096 bins)
    // 49.7-49.9 ms per clean forked after round 3 / delay 1, 48.2 after
    // round 4 / delay 2 (round 5: 48.4-48.7, 6: 49.1)
    if (!s->fftded && nbin >= 2048) {
        s->diag_fork = 4;
        s->fork_delay = 2;
    }
    // the fit cube (written by k_chan_partials mode 3, or by k_rotate in the FFT
    // mode) is tiled; IC_OPT_FIT_TILED = 0: row-major.  The closed-form fit of
    // the FFT mode reads its rotated fit cube row by row (k_diag DIAG_FIT).
    s->dtiled = (s->fftded && !exact) ? 0 : 1;
    if (s->fftded) {
        AL(s->dr, N);
        AL(s->Tc, N);
        // R (the rotated residual rows) only when a run measures them in a
        // separate pass (run_impl: !rot_stats_on)
        AL(s->zbase, P);
        AL(s->zshift, (size_t)nchan);
        AL(s->ph, 2 * (size_t)nchan * (nbin / 2 + 1));
        if (czt) {
            const std::vector<float> ct = czt_tables(nbin);
            AL(s->czt, ct.size());
            if (hipMemcpy(s->czt, ct.data(), sizeof(float) * ct.size(), hipMemcpyHostToDevice) != hipSuccess)
                return bail(fail(IC_EHIP, "upload of the chirp-z tables failed"));
        }
        if (hipMemset(s->zbase, 0, sizeof(float) * P) != hipSuccess ||
            hipMemset(s->zshift, 0, sizeof(int32_t) * nchan) != hipSuccess)
            return bail(fail(IC_EHIP, "hipMemset(zero levels / shifts) failed"));
    }
    AL(s->slot_w0[0], P);
    s->w0 = s->slot_w0[0];
    AL(s->W, P);
    AL(s->base, P);
    AL(s->base0, P);
    AL(s->valid, P);
    AL(s->slot_shift[0], (size_t)nchan);
    s->shift = s->slot_shift[0];
    AL(s->win, (size_t)nsub);
    AL(s->wflag, (size_t)nsub + 1);   // + window-moves counter
    AL(s->part, (size_t)nsub * s->nsb * nbin);
    // the incremental template stage's column flags (IC_OPT_TEMPLATE_INCR)
    AL(s->exA, (size_t)nsub * s->nsb * nbin);
    AL(s->exF, (size_t)nsub * s->nsb * nbin);
    AL(s->part2, (size_t)nsub * s->nsb * nbin);
    AL(s->wpart, (size_t)nsub * s->nsb);
    AL(s->F, (size_t)nsub * nbin);
    AL(s->wf, (size_t)nsub);
    AL(s->T, (size_t)nbin);
    AL(s->T64, (size_t)s->ldD);
    if (hipMemset(s->T64, 0, sizeof(double) * s->ldD) != hipSuccess)
        return bail(fail(IC_EHIP, "hipMemset(T64) failed"));   // zero tail: padded samples are no-ops
    AL(s->T2, (size_t)2 * nbin);
    AL(s->amp, P);
    AL(s->info, P);
    AL(s->std_, P);
    AL(s->mean, P);
    AL(s->ptp, P);
    AL(s->fft, P);
    AL(s->test, P);
    AL(s->hist, P * (size_t)(p.max_iter + 1));
    AL(s->lstat, (size_t)16 * (nchan + nsub));
    AL(s->tw, (size_t)nbin);
    AL(s->tw_p2, (size_t)nbin);
    AL(s->plan, 1);
    if (diag_czt_supported(nbin)) {
        const std::vector<double2> dt = diag_czt_tables(nbin);
        AL(s->dczt, dt.size());
        if (hipMemcpy(s->dczt, dt.data(), sizeof(double2) * dt.size(), hipMemcpyHostToDevice) != hipSuccess)
            return bail(fail(IC_EHIP, "upload of the chirp-z statistics tables failed"));
    }
    if (exact) AL(s->lists, 3 * P);   // two ping-pong round lists + the fork round's survivors
    AL(s->rcount, (size_t)kRoundWords + 4);   // + two spare words and the tail's sweep counter
    if (exact) AL(s->late, P);
    if (exact) {
        AL(s->tmark, P);
        if (hipMemset(s->tmark, 0, P) != hipSuccess) return bail(fail(IC_EHIP, "hipMemset(tail marks) failed"));
    }
    if (sharded) {
        std::string cerr;
        int ccode = IC_EINVAL;
        s->comm = make_comm(&cerr, &ccode);
        if (!s->comm) return bail(fail(ccode, "shard transport: %s", cerr.empty() ? "failed" : cerr.c_str()));
        s->comm->set_timeout_ms((long long)(s->sync_timeout_s * 1000.0 + 0.5));
        const size_t nchan_g = (size_t)p.nchan;
        AL(s->std_r, (size_t)s->rows_own * nchan_g);
        AL(s->mean_r, (size_t)s->rows_own * nchan_g);
        AL(s->fft_r, (size_t)s->rows_own * nchan_g);
        AL(s->ptp_r, (size_t)s->rows_own * nchan_g);
        AL(s->valid_r, (size_t)s->rows_own * nchan_g);
        size_t dsend = 0, drecv = 0;
        for (int r = 0; r < world; ++r) {
            const size_t rows_r = (size_t)(rr[2 * r + 1] - rr[2 * r]);
            const size_t nch_r = (size_t)(cr[2 * r + 1] - cr[2 * r]);
            s->dsb.push_back(shard_block_bytes(rows_r * nchan, 32));
            s->vsb.push_back(shard_block_bytes(rows_r * nchan, 1));
            s->drb.push_back(shard_block_bytes((size_t)s->rows_own * nch_r, 32));
            s->vrb.push_back(shard_block_bytes((size_t)s->rows_own * nch_r, 1));
            dsend += s->dsb.back();
            drecv += s->drb.back();
        }
        // root rows to their owners: rank r's block = its rows, contiguous in the send buffer
        for (int r = 0; r < world; ++r) {
            const size_t rows_r = (size_t)(rr[2 * r + 1] - rr[2 * r]);
            s->wsb.push_back(sizeof(double) * rows_r * nbin);
            s->wrb.push_back(sizeof(double) * s->rows_own * nbin);
            s->fsb.push_back(sizeof(double) * rows_r * (nbin + 1));
            s->frb.push_back(sizeof(double) * s->rows_own * (nbin + 1));
        }
        s->wg_blk = (s->rows_pad + 1) & ~1;
        s->fg_blk = ((long)s->rows_pad * (nbin + 1) + 1) & ~1L;
        struct {
            void **ptr;
            size_t bytes;
            const char *name;
        } xb[] = {{(void **)&s->xw_send, sizeof(double) * nsub * nbin, "window roots"},
                  {(void **)&s->xw_recv, sizeof(double) * world * s->rows_own * nbin, "owned window roots"},
                  {(void **)&s->xf_send, sizeof(double) * nsub * (nbin + 1), "fscrunch roots"},
                  {(void **)&s->xf_recv, sizeof(double) * world * s->rows_own * (nbin + 1), "owned fscrunch roots"},
                  {(void **)&s->xwg_send, sizeof(int32_t) * s->wg_blk, "owned windows"},
                  {(void **)&s->xwg_recv, sizeof(int32_t) * s->wg_blk * world, "gathered windows"},
                  {(void **)&s->xfg_send, sizeof(float) * s->fg_blk, "owned fscrunch rows"},
                  {(void **)&s->xfg_recv, sizeof(float) * s->fg_blk * world, "gathered fscrunch rows"},
                  {(void **)&s->xd_send, dsend, "diagnostics send"},
                  {(void **)&s->xd_recv, drecv, "diagnostics receive"},
                  {(void **)&s->xr_send, sizeof(double) * 8 * s->rows_pad, "row statistics"},
                  {(void **)&s->xr_recv, sizeof(double) * 8 * s->rows_pad * world, "gathered row statistics"},
                  // + 2: the standard template's hash words (run_impl), summed with the counters
                  {(void **)&s->counters, sizeof(int32_t) * (p.max_iter + 7), "counters"}};
        for (auto &b : xb)
            if (s->comm->alloc(b.ptr, b.bytes + 16) != 0 || !*b.ptr)
                return bail(fail(IC_ENOMEM, "exchange buffer (%s, %zu bytes) failed", b.name, b.bytes));
    } else {
        AL(s->counters, (size_t)(p.max_iter + 5));
    }
#undef AL
    if (hipHostMalloc((void **)&s->h_rcount, sizeof(int32_t) * kMaxRounds,
                      hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void **)&s->d_h_rcount, s->h_rcount, 0) != hipSuccess)
        return bail(fail(IC_ENOMEM, "hipHostMalloc(round counts) failed"));
    if (hipEventCreateWithFlags(&s->sev, hipEventDisableTiming) != hipSuccess)
        return bail(fail(IC_EHIP, "hipEventCreate failed"));
    if (hipHostMalloc((void **)&s->h_small, sizeof(int32_t) * ((size_t)p.max_iter + 24)) != hipSuccess)
        return bail(fail(IC_ENOMEM, "hipHostMalloc(readback) failed"));
    if (exact) {
        // fit state: 21 double arrays + 5 four-byte arrays, each padded to 256 B
        const size_t dstride = ((P * 8 + 255) / 256) * 256, istride = ((P * 4 + 255) / 256) * 256;
        if (s->mem.alloc_bytes(&s->fs_block, 21 * dstride + 5 * istride) != hipSuccess)
            return bail(fail(IC_ENOMEM, "hipMalloc(fit state) failed"));
        char *b = (char *)s->fs_block;
        double **dp[] = {&s->fs.x,     &s->fs.fnorm, &s->fs.par,   &s->fs.delta,   &s->fs.diag, &s->fs.xnorm,
                         &s->fs.acnorm, &s->fs.J0,   &s->fs.f0,    &s->fs.aj,      &s->fs.r,    &s->fs.Jn0,
                         &s->fs.qtf,   &s->fs.gnorm, &s->fs.x2,    &s->fs.pnorm,   &s->fs.wa1,  &s->fs.xa,
                         &s->fs.o_fnorm, &s->fs.o_acnorm, &s->fs.o_sum};
        for (auto *q : dp) { *q = (double *)b; b += dstride; }
        int32_t **ip[] = {&s->fs.iter, &s->fs.nfev, &s->fs.mode, &s->fs.slow, (int32_t **)&s->fs.p0};
        for (auto *q : ip) { *q = (int32_t *)b; b += istride; }
        s->fs.T64 = s->T64;
        // k_fit_prep's 4 scalars
        if (s->mem.alloc(&s->fs.U, 8) != hipSuccess) return bail(fail(IC_ENOMEM, "hipMalloc(fit prep) failed"));
    }
    // twiddles and the pairwise plan
    const std::vector<double2> tw = host_twiddles(nbin), tw2 = p2_twiddles(nbin);
    PwPlan plan;
    if (make_plan(nbin, &plan) != 0) return bail(fail(IC_EINVAL, "pairwise plan too large for nbin=%d", nbin));
    s->plan_ub = std::max(plan.nleaf, plan.nops);
    if (hipMemcpy(s->tw, tw.data(), sizeof(double2) * nbin, hipMemcpyHostToDevice) != hipSuccess ||
        (!tw2.empty() &&
         hipMemcpy(s->tw_p2, tw2.data(), sizeof(double2) * tw2.size(), hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemcpy(s->plan, &plan, sizeof plan, hipMemcpyHostToDevice) != hipSuccess)
        return bail(fail(IC_EHIP, "upload of constants failed"));
    *out = s;
    return IC_OK;
}

}  // namespace

extern "C" {

int ic_session_create(const ic_params *params, int device, void **out)
{
    return create_session(params, device, 0, 1, false, [](std::string *, int *) -> Comm * { return nullptr; }, out);
}

int ic_shard_layout(int nsub, int nchan, int world, int32_t *chan_ranges, int32_t *row_ranges)
{
    if (!chan_ranges || !row_ranges || nsub <= 0 || nchan <= 0) return fail(IC_EINVAL, "bad argument");
    if (const char *e = shard_layout(nsub, nchan, world, chan_ranges, row_ranges))
        return fail(IC_EINVAL, "cannot shard nchan=%d over %d: %s", nchan, world, e);
    return IC_OK;
}

int ic_session_create_shard(const ic_params *params, int device, int rank, int world, const ic_comm_ops *ops,
                            void **out)
{
    if (!ops || !ops->alloc || !ops->release || !ops->allgather || !ops->alltoallv || !ops->allreduce_sum_i32)
        return fail(IC_EINVAL, "incomplete ic_comm_ops");
    const ic_comm_ops o = *ops;
    return create_session(params, device, rank, world, true,
                          [&](std::string *, int *) -> Comm * { return make_callback_comm(o, rank, world); }, out);
}

int ic_rccl_unique_id(void *id_out)
{
    if (!id_out) return fail(IC_EINVAL, "null argument");
    std::string err;
    if (rccl_unique_id(id_out, &err)) return fail(IC_ECOMM, "ncclGetUniqueId: %s", err.c_str());
    return IC_OK;
}

int ic_rccl_set_library(const char *path)
{
    const char *err = nullptr;
    if (rccl_set_library(path, &err)) return fail(IC_ESTATE, "%s", err);
    return IC_OK;
}

int ic_rccl_set_init_timeout(int64_t ms)
{
    const char *err = nullptr;
    if (rccl_set_init_timeout((long long)ms, &err)) return fail(IC_EINVAL, "%s", err);
    return IC_OK;
}

int ic_session_create_rccl(const ic_params *params, int device, int rank, int world, const void *unique_id,
                           void **out)
{
    if (!unique_id) return fail(IC_EINVAL, "null unique id");
    return create_session(params, device, rank, world, true,
                          [&](std::string *err, int *code) -> Comm * {
                              *code = IC_ECOMM;   // librccl missing, a rank that never joined, RCCL's own errors
                              return make_rccl_comm(unique_id, rank, world, err);
                          },
                          out);
}

int ic_group_create(int world, void **group)
{
    if (!group) return fail(IC_EINVAL, "null argument");
    *group = local_group_create(world);
    if (!*group) return fail(IC_EINVAL, "bad group size %d", world);
    return IC_OK;
}

void ic_group_destroy(void *group) { local_group_destroy((LocalGroup *)group); }

int ic_session_create_grouped(const ic_params *params, int device, void *group, int rank, void **out)
{
    LocalGroup *g = (LocalGroup *)group;
    if (!g) return fail(IC_EINVAL, "null group");
    return create_session(params, device, rank, local_group_world(g), true,
                          [&](std::string *err, int *) -> Comm * {
                              const char *e = nullptr;
                              Comm *c = make_local_comm(g, rank, device, &e);
                              if (e) *err = e;
                              return c;
                          }, out);
}

void ic_session_destroy(void *session)
{
    Session *s = (Session *)session;
    if (!s) return;
    if (s->failed) {
        // kernels of this session may still be running (a wait timed out):
        // freeing their buffers could hand memory in use to another
        // allocation, and a synchronising free could hang; leak them.
        // Hazard (d) on this path: a residual download still queued writes the
        // caller's arrays, which the caller frees next, so it is waited for,
        // within the session's timeout (it sits behind those kernels)
        if (s->dl_pending && hipSetDevice(s->device) == hipSuccess) (void)poll_event(s, s->dl_ev);
        s->mem.abandon();
        delete s;
        return;
    }
    (void)hipSetDevice(s->device);
    free_all(s);
    delete s;
}

static int check_shifts(const Session *s, const int32_t *shift)
{
    for (int c = 0; c < s->nchan; ++c)
        if (shift[c] < 0 || shift[c] >= s->p.nbin) return fail(IC_EINVAL, "shift[%d]=%d out of [0,nbin)", c, shift[c]);
    return IC_OK;
}

// the end of every synchronous upload: the archive is the session's current one
static int finish_upload(Session *s)
{
    CK(hipStreamSynchronize(s->stream));
    s->uploaded = true;
    s->ran = false;
    s->hb_done = s->hb_have = false;
    return IC_OK;
}

// The input slot of the next asynchronous upload, the one not holding the
// newest data (after the queued upload, else after the current archive), made
// ready: the second slot is allocated at first need, as are the copy stream
// and the slot's event.
static int async_slot(Session *s, int *target)
{
    const int t = s->fifo_n ? 1 - s->fifo[s->fifo_n - 1] : (s->ever_uploaded ? 1 - s->cur : s->cur);
    if (s->mem.ensure(&s->slot_raw[t], s->N) != hipSuccess || s->mem.ensure(&s->slot_w0[t], s->P) != hipSuccess ||
        s->mem.ensure(&s->slot_shift[t], (size_t)s->nchan) != hipSuccess)
        return fail(IC_ENOMEM, "second input slot (%zu bytes) failed", sizeof(float) * (s->N + s->P));
    if (!s->copy_stream) CK(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
    if (!s->slot_ev[t]) CK(hipEventCreateWithFlags(&s->slot_ev[t], hipEventDisableTiming));
    // hazard (a): the run that used slot t has returned, but the residual encode
    // queued after it (ic_get_residual_quantised_async) may not have run yet, and
    // it reads the slot's shifts and, for the closed form, its raw cube: the
    // copies into the slot wait for the encode's event
    if (s->enc_slot == t) {
        CK(hipStreamWaitEvent(s->copy_stream, s->enc_ev, 0));
        s->enc_slot = -1;
    }
    *target = t;
    return IC_OK;
}

int ic_upload(void *session, const float *cube, const float *w0, const int32_t *shift)
{
    Session *s = (Session *)session;
    if (!s || !cube || !w0 || !shift) return fail(IC_EINVAL, "null argument");
    if (s->failed) return failed_session();
    if (s->fifo_n) return fail(IC_ESTATE, "ic_upload with %d asynchronous upload(s) pending", s->fifo_n);
    CK(hipSetDevice(s->device));
    if (int rc = check_shifts(s, shift)) return rc;
    s->ever_uploaded = true;
    CK(hipMemcpyAsync(s->raw, cube, sizeof(float) * s->N, hipMemcpyHostToDevice, s->stream));
    CK(hipMemcpyAsync(s->w0, w0, sizeof(float) * s->P, hipMemcpyHostToDevice, s->stream));
    CK(hipMemcpyAsync(s->shift, shift, sizeof(int32_t) * s->nchan, hipMemcpyHostToDevice, s->stream));
    return finish_upload(s);
}

int ic_upload_pols(void *session, const float *data, int npol, const float *w0, const int32_t *shift)
{
    Session *s = (Session *)session;
    if (!s || !data || !w0 || !shift) return fail(IC_EINVAL, "null argument");
    if (s->failed) return failed_session();
    if (npol < 1) return fail(IC_EINVAL, "npol=%d", npol);
    if (s->fifo_n) return fail(IC_ESTATE, "ic_upload_pols with %d asynchronous upload(s) pending", s->fifo_n);
    CK(hipSetDevice(s->device));
    if (int rc = check_shifts(s, shift)) return rc;
    s->ever_uploaded = true;
    const size_t row = sizeof(float) * (size_t)s->nchan * s->p.nbin;   // one subint of one polarisation
    // pol 0 -> raw; pol 1 -> the fit-cube buffer as scratch (rebuilt, and re-zeroed, below),
    // or a temporary buffer when the session keeps no fit cube (fit_mode 1)
    CK(hipMemcpy2DAsync(s->raw, row, data, row * npol, row, s->p.nsub, hipMemcpyHostToDevice, s->stream));
    if (npol >= 2) {
        const auto bad = [](hipError_t e) { return named_fail("ic_upload_pols", e); };
        Scratch tmp;
        float *pol1 = s->D;
        if (!pol1 && tmp.mem.alloc_exact(&pol1, s->N) != hipSuccess)
            return fail(IC_ENOMEM, "hipMalloc(pol1 scratch, %zu floats) failed", s->N);
        CKF(hipMemcpy2DAsync(pol1, row, (const char *)data + row, row * npol, row, s->p.nsub, hipMemcpyHostToDevice,
                             s->stream), bad);
        CKF(launch_pscrunch(s->stream, s->raw, pol1, s->N, s->grid_cap), bad);
        if (s->D)
            CKF(hipMemsetAsync(s->D, 0, sizeof(float) * s->Ppad * (size_t)s->ldD, s->stream), bad);
        else
            CKF(hipStreamSynchronize(s->stream), bad);   // pscrunch has read pol1 before tmp frees it
    }
    CK(hipMemcpyAsync(s->w0, w0, sizeof(float) * s->P, hipMemcpyHostToDevice, s->stream));
    CK(hipMemcpyAsync(s->shift, shift, sizeof(int32_t) * s->nchan, hipMemcpyHostToDevice, s->stream));
    return finish_upload(s);
}

int ic_upload_device(void *session, const float *d_cube, const float *d_w0, const int32_t *d_shift)
{
    Session *s = (Session *)session;
    if (!s || !d_cube || !d_w0 || !d_shift) return fail(IC_EINVAL, "null argument");
    if (s->failed) return failed_session();
    if (s->fifo_n) return fail(IC_ESTATE, "ic_upload_device with %d asynchronous upload(s) pending", s->fifo_n);
    CK(hipSetDevice(s->device));
    s->ever_uploaded = true;
    CK(hipMemcpyAsync(s->raw, d_cube, sizeof(float) * s->N, hipMemcpyDeviceToDevice, s->stream));
    CK(hipMemcpyAsync(s->w0, d_w0, sizeof(float) * s->P, hipMemcpyDeviceToDevice, s->stream));
    CK(hipMemcpyAsync(s->shift, d_shift, sizeof(int32_t) * s->nchan, hipMemcpyDeviceToDevice, s->stream));
    return finish_upload(s);
}

int ic_upload_async(void *session, const float *cube, const float *w0, const int32_t *shift)
{
    Session *s = (Session *)session;
    if (!s || !cube || !w0 || !shift) return fail(IC_EINVAL, "null argument");
    if (s->failed) return failed_session();
    if (s->fifo_n == 2) return fail(IC_ESTATE, "two asynchronous uploads already pending (run one first)");
    if (int rc = check_shifts(s, shift)) return rc;
    CK(hipSetDevice(s->device));
    int target = 0;
    if (int rc = async_slot(s, &target)) return rc;
    CK(hipMemcpyAsync(s->slot_raw[target], cube, sizeof(float) * s->N, hipMemcpyHostToDevice, s->copy_stream));
    CK(hipMemcpyAsync(s->slot_w0[target], w0, sizeof(float) * s->P, hipMemcpyHostToDevice, s->copy_stream));
    CK(hipMemcpyAsync(s->slot_shift[target], shift, sizeof(int32_t) * s->nchan, hipMemcpyHostToDevice,
                      s->copy_stream));
    CK(hipEventRecord(s->slot_ev[target], s->copy_stream));
    s->fifo[s->fifo_n++] = target;
    s->ever_uploaded = true;
    return IC_OK;
}

// arguments shared by the quantised entry points
static int q_check_args(const void *q, const float *scl, const float *offs, int npol, int nsum, int flags)
{
    if (!q || !scl || !offs) return fail(IC_EINVAL, "null argument");
    if (npol < 1) return fail(IC_EINVAL, "npol=%d", npol);
    if (nsum != 1 && nsum != 2) return fail(IC_EINVAL, "nsum=%d (1: pol 0, 2: pol 0 + pol 1)", nsum);
    if (nsum > npol) return fail(IC_EINVAL, "nsum=%d > npol=%d", nsum, npol);
    return check_q_flags(flags);
}

// the first nsum polarisations of every subint of host[nsub][npol][row bytes]
// -> dev[nsub][nsum][row bytes]
static hipError_t q_copy_pols(void *dev, const void *host, size_t row, int nsub, int npol, int nsum, hipStream_t st)
{
    if (nsum == npol) return hipMemcpyAsync(dev, host, row * nsum * nsub, hipMemcpyHostToDevice, st);
    return hipMemcpy2DAsync(dev, row * nsum, host, row * npol, row * nsum, nsub, hipMemcpyHostToDevice, st);
}

// staging of one slot for nsum polarisations.  A slot being (re)allocated holds
// no pending upload and the decode of any earlier one has been waited for by
// the ic_run that consumed it, so freeing the smaller staging is safe.
static int q_stage(Session *s, int slot, int nsum)
{
    if (s->slot_qsum[slot] >= nsum) return IC_OK;
    s->mem.release(s->slot_q[slot]);
    s->mem.release(s->slot_so[slot]);
    s->slot_qsum[slot] = 0;
    if (s->mem.alloc(&s->slot_q[slot], s->N * nsum) != hipSuccess ||
        s->mem.alloc(&s->slot_so[slot], s->P * 2 * nsum) != hipSuccess)
        return fail(IC_ENOMEM, "quantised staging (%zu bytes) failed",
                    (size_t)nsum * (sizeof(int16_t) * s->N + 2 * sizeof(float) * s->P));
    s->slot_qsum[slot] = nsum;
    return IC_OK;
}

// copies and decode of one quantised archive into input slot `slot`, on `st`
static int q_enqueue(Session *s, int slot, hipStream_t st, const int16_t *q, const float *scl, const float *offs,
                     int npol, int nsum, int flags, const float *w0, const int32_t *shift)
{
    const int nsub = s->p.nsub, nchan = s->nchan, nbin = s->p.nbin;
    float *dscl = s->slot_so[slot], *doffs = dscl + s->P * nsum;
    CK(q_copy_pols(s->slot_q[slot], q, sizeof(int16_t) * (size_t)nchan * nbin, nsub, npol, nsum, st));
    CK(q_copy_pols(dscl, scl, sizeof(float) * (size_t)nchan, nsub, npol, nsum, st));
    CK(q_copy_pols(doffs, offs, sizeof(float) * (size_t)nchan, nsub, npol, nsum, st));
    CK(launch_decode_q(st, s->slot_q[slot], dscl, doffs, nsub, nchan, nbin, nsum, (flags & IC_Q_BIG_ENDIAN) != 0,
                       s->slot_raw[slot], s->grid_cap));
    CK(hipMemcpyAsync(s->slot_w0[slot], w0, sizeof(float) * s->P, hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(s->slot_shift[slot], shift, sizeof(int32_t) * nchan, hipMemcpyHostToDevice, st));
    return IC_OK;
}

int ic_upload_quantised(void *session, const int16_t *q, const float *scl, const float *offs, int npol, int nsum,
                        int flags, const float *w0, const int32_t *shift)
{
    Session *s = (Session *)session;
    if (!s || !w0 || !shift) return fail(IC_EINVAL, "null argument");
    if (int rc = q_check_args(q, scl, offs, npol, nsum, flags)) return rc;
    if (s->failed) return failed_session();
    if (s->fifo_n) return fail(IC_ESTATE, "ic_upload_quantised with %d asynchronous upload(s) pending", s->fifo_n);
    CK(hipSetDevice(s->device));
    if (int rc = check_shifts(s, shift)) return rc;
    if (int rc = q_stage(s, s->cur, nsum)) return rc;
    s->ever_uploaded = true;
    if (int rc = q_enqueue(s, s->cur, s->stream, q, scl, offs, npol, nsum, flags, w0, shift)) return rc;
    return finish_upload(s);
}

int ic_upload_quantised_async(void *session, const int16_t *q, const float *scl, const float *offs, int npol, int nsum,
                              int flags, const float *w0, const int32_t *shift)
{
    Session *s = (Session *)session;
    if (!s || !w0 || !shift) return fail(IC_EINVAL, "null argument");
    if (int rc = q_check_args(q, scl, offs, npol, nsum, flags)) return rc;
    if (s->failed) return failed_session();
    if (s->fifo_n == 2) return fail(IC_ESTATE, "two asynchronous uploads already pending (run one first)");
    if (int rc = check_shifts(s, shift)) return rc;
    CK(hipSetDevice(s->device));
    int target = 0;
    if (int rc = async_slot(s, &target)) return rc;
    if (int rc = q_stage(s, target, nsum)) return rc;
    // the decode runs on the copy stream behind its copies and slot_ev follows
    // it: ic_run waits for a decoded cube as it waits for an f32 copy
    if (int rc = q_enqueue(s, target, s->copy_stream, q, scl, offs, npol, nsum, flags, w0, shift)) return rc;
    CK(hipEventRecord(s->slot_ev[target], s->copy_stream));
    s->fifo[s->fifo_n++] = target;
    s->ever_uploaded = true;
    return IC_OK;
}

int ic_decode_profiles(int device, int nsub, int npol, int nsum, int nchan, int nbin, const int16_t *q,
                       const float *scl, const float *offs, int flags, float *out)
{
    if (!out) return fail(IC_EINVAL, "null argument");
    if (int rc = q_check_args(q, scl, offs, npol, nsum, flags)) return rc;
    if (nsub <= 0 || nchan <= 0 || nbin <= 0) return fail(IC_EINVAL, "bad shape (%d, %d, %d)", nsub, nchan, nbin);
    if (int rc = select_device(device)) return rc;
    const size_t P = (size_t)nsub * nchan, N = P * nbin;
    const auto bad = [](hipError_t e) { return named_fail("ic_decode_profiles", e, true); };
    Scratch sc;
    int16_t *dq = nullptr;
    float *dso = nullptr, *d = nullptr;
    CKF(sc.open_stream(), bad);
    hipStream_t st = sc.stream;
    CKF(sc.mem.alloc_exact(&dq, N * nsum), bad);
    CKF(sc.mem.alloc_exact(&dso, P * 2 * nsum), bad);
    CKF(sc.mem.alloc_exact(&d, N), bad);
    CKF(q_copy_pols(dq, q, sizeof(int16_t) * (size_t)nchan * nbin, nsub, npol, nsum, st), bad);
    CKF(q_copy_pols(dso, scl, sizeof(float) * (size_t)nchan, nsub, npol, nsum, st), bad);
    CKF(q_copy_pols(dso + P * nsum, offs, sizeof(float) * (size_t)nchan, nsub, npol, nsum, st), bad);
    CKF(launch_decode_q(st, dq, dso, dso + P * nsum, nsub, nchan, nbin, nsum, (flags & IC_Q_BIG_ENDIAN) != 0, d), bad);
    CKF(hipMemcpyAsync(out, d, sizeof(float) * N, hipMemcpyDeviceToHost, st), bad);
    CKF(hipStreamSynchronize(st), bad);
    return IC_OK;
}

int ic_host_alloc(size_t bytes, void **ptr)
{
    if (!ptr) return fail(IC_EINVAL, "null argument");
    *ptr = nullptr;
    if (hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess || !*ptr)
        return fail(IC_ENOMEM, "hipHostMalloc(%zu) failed", bytes);
    return IC_OK;
}

void ic_host_free(void *ptr)
{
    if (ptr) (void)hipHostFree(ptr);
}

int ic_set_timing_kernel(void *session, int kernel)
{
    Session *s = (Session *)session;
    if (!s) return fail(IC_EINVAL, "null session");
    if (s->failed) return failed_session();
    if (kernel >= K_COUNT) return fail(IC_EINVAL, "kernel id %d >= %d", kernel, (int)K_COUNT);
    s->timing_only = kernel < 0 ? -1 : kernel;
    return IC_OK;
}

int ic_set_timing(void *session, int enabled)
{
    Session *s = (Session *)session;
    if (!s) return fail(IC_EINVAL, "null session");
    if (s->failed) return failed_session();
    s->timing = enabled != 0;
    s->events.clear();   // events of earlier runs are discarded unread
    s->enext = 0;
    for (int q = 0; q < K_COUNT; ++q) {
        s->kms[q] = 0.0;
        s->klaunch[q] = 0;
    }
    return IC_OK;
}

int ic_get_kernel_times(void *session, ic_kernel_time *out, int n)
{
    Session *s = (Session *)session;
    if (!s || (!out && n > 0)) return fail(IC_EINVAL, "null argument");
    if (s->failed) return failed_session();
    if (int rc = collect_timing(s)) return rc;
    int m = 0;
    for (int q = 0; q < K_COUNT && m < n; ++q) {
        out[m].kernel = q;
        out[m].launches = s->klaunch[q];
        out[m].ms = s->kms[q];
        ++m;
    }
    return m;
}

}  // extern "C"

namespace {

// the diagnostics launch of one iteration: exact fit (amp/info from run_fit,
// fit cube D) or closed form (k_diag computes amp/info from raw and base0)
DiagArgs diag_args(Session *s, int pr_start, int pr_end)
{
    const ic_params &p = s->p;
    DiagArgs a{};
    a.mode = p.fit_mode == IC_FIT_EXACT ? DIAG_EXACT : DIAG_CLOSED;
    a.D = s->D;
    a.ldD = s->ldD;
    a.dtiled = s->dtiled;
    a.raw = s->raw;
    a.base = s->base0;
    a.T64 = s->T64;
    a.T2 = s->T2;
    a.TT = s->TT;
    a.amp = s->amp;
    a.info = s->info;
    a.w0 = s->w0;
    a.shift = s->shift;
    a.tw = s->tw;
    a.tw_p2 = s->tw_p2;
    a.plan = s->plan;
    a.nsub = p.nsub;
    a.nchan = s->nchan;
    a.nbin = p.nbin;
    a.pr_on = p.pr_on;
    a.pr_factor = p.pr_factor;
    a.pr_start = pr_start;
    a.pr_end = pr_end;
    a.std_o = s->std_;
    a.mean_o = s->mean;
    a.fft_o = s->fft;
    a.ptp_o = s->ptp;
    a.data_f64 = p.data_f64 != 0;
    a.chain = s->diag_chain ? 1 : 0;
    a.grid_cap = s->grid_cap;
    a.czt = s->dczt;
    return a;
}

// ---- piecewise detrending: the pieces of a direction (ic_set_detrend_pieces) ----
// starts[0..np) of lines of n entries; np == 0 with no pointer: one piece.
// 0 or the message
const char *pieces_range(int np, const int32_t *starts, int n)
{
    if (np < 0 || np > kMaxPieces) return "npieces outside 0..512";
    if (np == 0) return nullptr;
    if (!starts) return "null starts with npieces > 0";
    if (starts[0] != 0) return "the first start is not 0";
    for (int q = 0; q < np; ++q) {
        if (q > 0 && starts[q] <= starts[q - 1]) return "starts not strictly ascending";
        if (starts[q] >= n) return "a start at or past the line's length";
    }
    return nullptr;
}

// the kernels' tables of checked pieces: both directions' starts, each list
// closed by its n, and the piece of every subint, then of every channel
struct PieceTables {
    std::vector<int32_t> starts;
    std::vector<int16_t> piece;
};
PieceTables piece_tables(const std::vector<int32_t> &cs, const std::vector<int32_t> &ss, int nsub, int nchan)
{
    PieceTables t;
    for (int dir = 0; dir < 2; ++dir) {
        const std::vector<int32_t> &b = dir ? ss : cs;
        const int n = dir ? nchan : nsub;
        t.starts.insert(t.starts.end(), b.begin(), b.end());
        t.starts.push_back(n);
        for (size_t q = 0; q < b.size(); ++q)
            t.piece.insert(t.piece.end(), (size_t)((q + 1 < b.size() ? b[q + 1] : n) - b[q]), (int16_t)q);
    }
    return t;
}
// the tables on the device (starts: cs.size() + ss.size() + 2 words; piece: nsub + nchan)
PieceArgs piece_args(const std::vector<int32_t> &cs, const std::vector<int32_t> &ss, int nsub, const int32_t *starts,
                     const int16_t *piece)
{
    return PieceArgs{(int)cs.size(), (int)ss.size(), starts, starts + cs.size() + 1, piece, piece + nsub};
}

// ---- hot-bin repair (ic_set_hotbins; hotbins.py) ----
// the on-pulse window in the kernels' form: (start, length), widened by one bin
// on each side for fractional delays (never from nothing, never beyond nbin)
void hot_window(int nbin, int on_start, int on_end, bool widen, int *start, int *len)
{
    int L = ((on_end - on_start) % nbin + nbin) % nbin, st = on_start;
    if (widen && L > 0) {
        st = (st + nbin - 1) % nbin;
        L = L + 2 < nbin ? L + 2 : nbin;
    }
    *start = st;
    *len = L;
}
// the ranges of ic_set_hotbins / ic_hotbins_profiles; 0 or the message
const char *hotbins_range(int nbin, double threshold, int on_start, int on_end, int rounds, bool widen)
{
    if (!(std::isfinite(threshold) && threshold > 0.0)) return "threshold must be finite and > 0";
    if (rounds < 1 || rounds > kHotMaxRounds) return "rounds outside 1..8";
    if (nbin > kHotMaxBin) return "nbin above 8192";
    if (on_start < 0 || on_start >= nbin) return "on_start outside [0, nbin)";
    if (on_end < 0 || on_end > nbin) return "on_end outside [0, nbin]";
    int ws = 0, wl = 0;
    hot_window(nbin, on_start, on_end, widen, &ws, &wl);
    if (nbin - wl < kHotMinOff) return "fewer than 8 off-pulse bins";
    return nullptr;
}
// fractional delays move the pulse by their rounded value and widen the window
bool hot_widen(const Session *s) { return s->fftded && !s->p.input_dedispersed; }

// the upload's one pass: detect and repair in place, then the rows' starts
int hotbins_stage(Session *s)
{
    const int nbin = s->p.nbin;
    const size_t words = (size_t)hot_mask_words(nbin);
    if (s->mem.ensure(&s->hb_count, s->P) != hipSuccess || s->mem.ensure(&s->hb_mask, s->P * words) != hipSuccess ||
        s->mem.ensure(&s->hb_offs, s->P) != hipSuccess ||
        s->mem.ensure(&s->hb_total, 1 + hotbin_scan_parts((long)s->P)) != hipSuccess)
        return fail(IC_ENOMEM, "hipMalloc(hot-bin counts and masks: %zu bytes) failed",
                    s->P * (12 + 4 * words));
    HotBinArgs a{};
    a.cube = s->raw;
    a.w0 = s->w0;
    const bool frac = hot_widen(s);
    if (frac) {
        a.offd = s->delay2 ? s->delay2 : s->dly;
        a.per_profile = s->delay2 ? 1 : 0;
        if (!a.offd) return fail(IC_ESTATE, "hot-bin repair: the session has no delays");
    } else if (!s->fftded) {
        a.off32 = s->shift;
    }
    a.P = (long)s->P;
    a.nchan = s->nchan;
    a.nbin = nbin;
    hot_window(nbin, s->hb_start, s->hb_end, frac, &a.win_start, &a.win_len);
    a.threshold = s->hb_thr;
    a.rounds = s->hb_rounds;
    a.count = s->hb_count;
    a.mask = s->hb_mask;
    a.grid_cap = s->grid_cap;
    LAUNCH(s, K_HOTBINS, launch_hotbins(s->stream, a));
    LAUNCH(s, K_HOTBIN_SCAN, launch_hotbin_scan(s->stream, s->hb_count, (long)s->P, s->hb_total + 1, s->hb_offs,
                                                s->hb_total));
    s->hb_done = s->hb_have = true;
    return IC_OK;
}

// ---- the line stage: medians / MADs along the lines, then combine ----
// a's line statistics over one lstat block of 8 (nsub + nchan) doubles
void lay_lstat(LineStatsArgs *a, int nsub, int nchan, double *lstat)
{
    a->nsub = nsub;
    a->nchan = nchan;
    a->col_med = lstat;
    a->col_mad = lstat + 4 * nchan;
    a->row_med = lstat + 8 * nchan;
    a->row_mad = lstat + 8 * nchan + 4 * nsub;
}

// a run's line stage: ta is read when detrend, pa when pieces
struct LineStage {
    LineStatsArgs la;
    TrendArgs ta;
    PieceArgs pa;
    bool detrend, pieces;
};

// once per run: the stage's arguments; what the detrended forms need is
// allocated (and the piece tables uploaded) at the first run that needs it
int line_stage_prepare(Session *s, LineStage *g)
{
    const ic_params &p = s->p;
    const int nsub = p.nsub, nchan = s->nchan;
    LineStatsArgs &la = g->la;
    lay_lstat(&la, nsub, nchan, s->lstat);
    la.valid = s->valid;
    la.std_d = s->std_;
    la.mean_d = s->mean;
    la.fft_d = s->fft;
    la.ptp_d = s->ptp;
    la.ptp_f32 = !p.data_f64;
    la.grp_waves = s->ls_knobs.grp_waves;
    la.grp_minlen = s->ls_knobs.grp_minlen;
    const bool detrend = g->detrend = s->dt_chan > 0 || s->dt_sub > 0;
    if (detrend && !s->pw_on && s->mem.ensure(&s->trend, (size_t)16 * (nchan + nsub)) != hipSuccess)
        return fail(IC_ENOMEM, "hipMalloc(trend coefficients: %zu doubles) failed", (size_t)16 * (nchan + nsub));
    g->ta = TrendArgs{s->dt_chan, s->dt_sub, s->dt_rounds, s->dt_clip, s->trend,
                      s->trend ? s->trend + (size_t)16 * nchan : nullptr};
    // piecewise (ic_set_detrend_pieces): its own tables and coefficient arrays
    const bool pieces = g->pieces = detrend && s->pw_on;
    g->pa = PieceArgs{};
    if (pieces) {
        const size_t mc = s->pw_cs.size(), ms = s->pw_ss.size();
        if (!s->pw_trend) {   // allocated last: set once all three are there
            // (a shard's subint pieces: those of the whole subint line, on every rank)
            const PieceTables pt = piece_tables(s->pw_cs, s->pw_ss, nsub, p.nchan);
            if (s->mem.ensure(&s->pw_starts, pt.starts.size()) != hipSuccess ||
                s->mem.ensure(&s->pw_piece, pt.piece.size()) != hipSuccess ||
                s->mem.ensure(&s->pw_trend, 16 * ((size_t)nchan * mc + (size_t)nsub * ms)) != hipSuccess)
                return fail(IC_ENOMEM, "hipMalloc(piecewise trends: %zu doubles) failed",
                            16 * ((size_t)nchan * mc + (size_t)nsub * ms));
            CK(hipMemcpyAsync(s->pw_starts, pt.starts.data(), sizeof(int32_t) * pt.starts.size(),
                              hipMemcpyHostToDevice, s->stream));
            CK(hipMemcpyAsync(s->pw_piece, pt.piece.data(), sizeof(int16_t) * pt.piece.size(), hipMemcpyHostToDevice,
                              s->stream));
            CK(hipStreamSynchronize(s->stream));   // pt goes out of scope
        }
        g->pa = piece_args(s->pw_cs, s->pw_ss, nsub, s->pw_starts, s->pw_piece);
        g->ta.col_coef = s->pw_trend;
        g->ta.row_coef = s->pw_trend + 16 * (size_t)nchan * mc;
    }
    // a shard's slots of detrended row statistics (shard_rowtrends): the
    // transport's, sized for this run's subint pieces
    if (detrend && s->comm) {
        if (!s->sh_dt) return fail(IC_ESTATE, "detrending on a channel shard without ic_shard_enable_detrend");
        const size_t ms = pieces ? s->pw_ss.size() : 1;
        if (s->xt_ms != ms) {
            s->comm->release(s->xt_send);
            s->comm->release(s->xt_recv);
            s->xt_send = s->xt_recv = nullptr;
            s->xt_ms = 0;
        }
        if (!s->xt_send) {
            const size_t slot = sizeof(double) * (size_t)s->rows_pad * (8 + 16 * ms);
            if (s->comm->alloc((void **)&s->xt_send, slot + 16) != 0 || !s->xt_send ||
                s->comm->alloc((void **)&s->xt_recv, slot * s->world + 16) != 0 || !s->xt_recv)
                return fail(IC_ENOMEM, "exchange buffer (row trends, %zu bytes gathered) failed", slot * s->world);
            s->xt_ms = ms;
        }
    }
    return 0;
}

// once per iteration: the lines, a shard's rows, the counters, combine
int line_stage(Session *s, const LineStage &g, int n_iter)
{
    const ic_params &p = s->p;
    const TrendArgs *ta = g.detrend ? &g.ta : nullptr;
    const PieceArgs *pa = g.pieces ? &g.pa : nullptr;
    // channel medians are local to a shard (detrended too: a channel line is
    // whole on its shard, ic_shard_enable_detrend); row medians need whole rows,
    // which their row owners take
    LAUNCH(s, K_LINESTATS, launch_lines(s->stream, g.la, ta, pa, s->comm ? 1 : 3));
    if (s->comm)
        if (int rc = ta ? shard_rowtrends(s, g.la, *ta, pa) : shard_rowstats(s, g.la)) return rc;
    // (a shard's counters end in the two words of the standard template's hash, run_impl)
    CK(hipMemsetAsync(s->counters, 0, sizeof(int32_t) * (p.max_iter + (s->comm ? 7 : 5)), s->stream));
    CombineArgs c;
    c.ls = g.la;
    c.info = s->info;
    c.w0 = s->w0;
    c.chanthresh = p.chanthresh;
    c.subintthresh = p.subintthresh;
    c.test = s->test;
    c.W = s->W;
    c.hist = s->hist;
    c.iter = n_iter;
    c.counters = s->counters;
    c.grid_cap = s->grid_cap;
    c.trend = ta;
    c.pieces = pa;
    if (ta && s->comm) {
        c.chan0 = s->c0;
        c.nchan_g = p.nchan;
    }
    LAUNCH(s, K_COMBINE, launch_combine(s->stream, c));
    return 0;
}

int run_impl(Session *s, double *test_out, float *weights_out, int32_t *loops_out, int32_t *changed_out,
             int32_t *nzero_out, int32_t *n_iter_out, int32_t *converged_out)
{
    CK(hipSetDevice(s->device));
    if (s->fifo_n) {   // the oldest asynchronous upload becomes the current archive
        const int slot = s->fifo[0];
        s->fifo[0] = s->fifo[1];
        --s->fifo_n;
        CK(hipStreamWaitEvent(s->stream, s->slot_ev[slot], 0));
        s->cur = slot;
        s->raw = s->slot_raw[slot];
        s->w0 = s->slot_w0[slot];
        s->shift = s->slot_shift[slot];
        s->uploaded = true;
        s->ran = false;
        s->hb_done = s->hb_have = false;
        // delays that came with the upload become the session's (slot_ev
        // follows their copy and the table kernel)
        if (s->slot_dmode[slot] == 1) {
            std::swap(s->ph, s->slot_ph[slot]);
            // ... and the channel row they were built from (the hot-bin pass
            // reads it for the profiles' offsets): the slot keeps the session's
            // old buffer, so a later upload into the slot overwrites nothing
            // the session still reads
            std::swap(s->dly, s->slot_dly[slot]);
            s->delay2 = nullptr;   // a per-channel archive after a per-profile one
        } else if (s->slot_dmode[slot] == 2) {
            std::swap(s->dly, s->slot_dly[slot]);
            s->delay2 = s->dly;
        }
        if (s->slot_dmode[slot]) s->delays_set = true;
        s->slot_dmode[slot] = 0;
    }
    if (!s->uploaded) return fail(IC_ESTATE, "ic_run before ic_upload");
    // timed launches of earlier runs: fold them into the totals so the event
    // pool stays at one run's worth (the previous run ended synchronised)
    if (s->events.size() > 4096)
        if (int rc = collect_timing(s)) return rc;
    if (s->fftded && !s->delays_set) return fail(IC_ESTATE, "ic_run before ic_set_delays (dedisp_mode FFT)");
    if (s->fftded && !rot_stats_on(s) && s->mem.ensure(&s->R, s->N) != hipSuccess)
        return fail(IC_ENOMEM, "hipMalloc(R: %zu floats) failed", s->N);
    // the second fork's tail marks are cleared at the end of each iteration; a
    // run that failed in between may have left some set
    if (s->tmark) CK(hipMemsetAsync(s->tmark, 0, s->P, s->stream));
    const ic_params &p = s->p;
    const int nsub = p.nsub, nbin = p.nbin;
    int pr_start = p.pr_start < 0 ? 0 : (p.pr_start > nbin ? nbin : p.pr_start);
    int pr_end = p.pr_end < 0 ? 0 : (p.pr_end > nbin ? nbin : p.pr_end);
    // fit cube (ic.py:96-100) + initial weights/history; a session can be re-run
    s->stats = ic_run_stats{};
    if (s->hb_on && !s->hb_done)
        if (int rc = hotbins_stage(s)) return rc;
    if (int rc = prepare(s)) return rc;
    s->trends_ran = false;
    s->std_ran = false;
    LineStage ls;
    if (int rc = line_stage_prepare(s, &ls)) return rc;
    int32_t *cnt = s->h_small;   // [max_iter + 5] counters, then the run stats (pinned)
    s->bad_fits.clear();
    int x = 0, loops = -1, n_iter = 0, converged = 0;
    // k_fit_tail's sweep counter (after the per-round counters): one run's total
    CK(hipMemsetAsync(tail_counter(s), 0, sizeof(unsigned long long), s->stream));
    while (x < p.max_iter) {
        x += 1;
        ++n_iter;
        if (int rc = iteration_template(s, n_iter)) return rc;
        if (s->std_on)
            if (int rc = std_stage(s)) return rc;
        DiagArgs da = diag_args(s, pr_start, pr_end);
        // the statistics pass: FFT dedispersion measures the residual rows
        // rotated back to the dispersed frame (R), written by k_rotate
        DiagArgs ds = da;
        if (s->fftded) {
            ds.mode = DIAG_STATS;
            ds.D = s->R;
            ds.ldD = nbin;
            ds.dtiled = 0;
        }
        s->pr_lo = pr_start;
        s->pr_hi = pr_end;
        if (p.fit_mode == IC_FIT_EXACT) {
            const bool fork = s->diag_fork > 0 && s->dstream && s->late && diag_list_supported(ds);
            if (int rc = run_fit(s, fork ? &ds : nullptr)) return rc;
        } else {
            LAUNCH(s, K_TNORM, launch_tnorm(s->stream, s->T64, s->plan, s->plan_ub, s->TT));
        }
        if (s->fftded) {
            if (p.fit_mode == IC_FIT_CLOSED) {   // the closed-form amplitudes of the rotated fit cube
                DiagArgs fa = da;
                fa.mode = DIAG_FIT;
                LAUNCH(s, K_DIAG, launch_diag(s->stream, fa));
            }
            // residual in the dedispersed frame, dededispersed by the inverse
            // rotation (ic.py:101-104), then comprehensive_stats of those rows
            // (after a fork: the profiles still fitting at it, the others were
            // rotated on dstream)
            RotateArgs ra = residual_rotate_args(s, pr_start, pr_end);
            if (s->fork_round >= 0) {
                // pass B: the profiles still fitting at the fork round.  With
                // per-profile delays from the round's survivor list (C2 fft_pp
                // 47.64-47.80 -> 47.24-47.34 ms per clean); with a channel's
                // phasor table by the late flags over the channel-major items,
                // whose profiles share the table row (the list: 45.44-45.57 ->
                // 45.77-45.88)
                if (s->delay2) {
                    ra.list = s->lists + 2 * s->P;
                    ra.nctr = (const unsigned long long *)s->rcount + s->fork_round;
                } else {
                    ra.late = s->late;
                    ra.late_sel = 1;
                }
            }
            if (rot_stats_on(s)) with_stats(s, ra);
            LAUNCH(s, K_ROTATE, launch_rotate(s->stream, ra));
            da = ds;
        }
        if (rot_stats_on(s)) {
            // the rotation measured its rows (after a fork: pass A's on dstream)
            if (s->fork_round >= 0) CK(hipStreamWaitEvent(s->stream, s->join_ev, 0));
        } else if (s->tail_split) {
            // the tail's profiles (the rest of pass B ran beside the tail), then
            // join dstream and clear the marks for the next iteration
            DiagArgs b = da;
            b.list = s->tail_list;
            b.nctr = s->tail_cin;
            LAUNCH(s, K_DIAG, launch_diag(s->stream, b));
            CK(hipStreamWaitEvent(s->stream, s->join_ev, 0));
            CK(launch_mark_list(s->stream, s->tail_list, s->tail_cin, (long)s->P, s->tail_bound, s->tmark, 0));
        } else if (s->fork_round >= 0) {
            // pass B: the profiles still fitting at the fork, then join pass A
            DiagArgs b = da;
            b.list = s->lists + 2 * s->P;
            b.nctr = (const unsigned long long *)s->rcount + s->fork_round;
            LAUNCH(s, K_DIAG, launch_diag(s->stream, b));
            CK(hipStreamWaitEvent(s->stream, s->join_ev, 0));
        } else {
            LAUNCH(s, K_DIAG, launch_diag(s->stream, da));
        }
        if (int rc = line_stage(s, ls, n_iter)) return rc;
        // a shard: two words of the standard template's hash (zero, as the
        // memset left them, when none is set; the first at least 1 otherwise)
        // ride behind the counters in the same all-reduce on every rank, so
        // that ranks which set different standards or modes, or of which only
        // some set one, are detected: each rank compares the sums with world
        // times its own words
        const int nhash = s->comm ? 2 : 0;
        int32_t *hw = s->h_small + p.max_iter + 14;   // pinned
        hw[0] = hw[1] = 0;
        if (nhash && s->std_on) {
            hw[0] = (int32_t)(s->std_hash & 0x7fffu) + 1;
            hw[1] = (int32_t)((s->std_hash >> 15) & 0x7fffu);
            CK(hipMemcpyAsync(s->counters + n_iter + 4, hw, sizeof(int32_t) * 2, hipMemcpyHostToDevice, s->stream));
        }
        if (s->comm)
            CM(s, s->comm->allreduce_sum_i32(s->counters, (size_t)(n_iter + 4 + nhash), s->stream),
               "convergence counters");
        CK(hipMemcpyAsync(cnt, s->counters, sizeof(int32_t) * (n_iter + 4 + nhash), hipMemcpyDeviceToHost,
                          s->stream));
        CK(spin_sync(s));
        if (nhash && (cnt[n_iter + 4] != s->world * hw[0] || cnt[n_iter + 5] != s->world * hw[1]))
            return fail(IC_EINVAL, "the ranks of this shard group set different standard templates or alignment "
                                   "modes, or only some set one (ic_set_std_template): every rank must set the same");
        if (changed_out) changed_out[n_iter - 1] = cnt[0];
        if (nzero_out) nzero_out[n_iter - 1] = cnt[1];
        s->bad_fits.push_back(cnt[2]);
        s->stats.near_threshold = cnt[3];
        for (int h = 0; h < n_iter; ++h)
            if (cnt[4 + h] == 0) {
                loops = x;
                converged = 1;
                x = 1000000;
            }
        if (s->std_on && !converged && p.max_iter >= 2) {
            // One pass: with a fixed template iteration 2 reads what iteration 1
            // read (D, w0, valid, T), so it would write the same diagnostics,
            // test values and weights, change nothing and end the loop.  It is
            // reported, not launched: its records repeat iteration 1's.
            CK(hipMemcpyAsync(s->hist + 2 * s->P, s->hist + s->P, sizeof(float) * s->P, hipMemcpyDeviceToDevice,
                              s->stream));
            ++n_iter;
            if (changed_out) changed_out[n_iter - 1] = 0;
            if (nzero_out) nzero_out[n_iter - 1] = cnt[1];
            s->bad_fits.push_back(cnt[2]);
            loops = 2;
            converged = 1;
            x = 1000000;
        }
    }
    if (x == p.max_iter) loops = p.max_iter;
    s->last_iter = n_iter;
    if (test_out && n_iter > 0)
        CK(hipMemcpyAsync(test_out, s->test, sizeof(double) * s->P, hipMemcpyDeviceToHost, s->stream));
    if (weights_out)
        CK(hipMemcpyAsync(weights_out, s->W, sizeof(float) * s->P, hipMemcpyDeviceToHost, s->stream));
    {
        int32_t *moves = s->h_small + p.max_iter + 6;                               // pinned
        unsigned long long *tsw = (unsigned long long *)(s->h_small + ((p.max_iter + 9) & ~1));   // 8-B aligned
        CK(hipMemcpyAsync(moves, s->wflag + nsub, sizeof *moves, hipMemcpyDeviceToHost, s->stream));
        CK(hipMemcpyAsync(tsw, tail_counter(s), sizeof *tsw, hipMemcpyDeviceToHost, s->stream));
        CK(spin_sync(s));
        s->stats.window_moves = *moves;
        s->stats.fit_tail_sweeps += (int64_t)tsw[0];
    }
    // timing events are read when asked for (ic_get_kernel_times), not here
    if (loops_out) *loops_out = loops;
    if (n_iter_out) *n_iter_out = n_iter;
    s->stats.iterations = n_iter;
    if (converged_out) *converged_out = converged;
    s->ran = n_iter > 0;
    s->trends_ran = ls.detrend && n_iter > 0;
    s->std_ran = s->std_on && n_iter > 0;
    return IC_OK;
}

}  // namespace

extern "C" {

int ic_run(void *session, double *test_out, float *weights_out, int32_t *loops_out, int32_t *changed_out,
           int32_t *nzero_out, int32_t *n_iter_out, int32_t *converged_out)
{
    Session *s = (Session *)session;
    if (!s) return fail(IC_EINVAL, "null session");
    if (s->failed) return failed_session();
    int rc = run_impl(s, test_out, weights_out, loops_out, changed_out, nzero_out, n_iter_out, converged_out);
    if (rc && s->comm_lost) rc = fail(IC_ECOMM, "the shard transport lost a peer (RCCL asynchronous error)");
    if (rc && s->comm) s->comm->abort();   // peers must not wait for this shard
    return rc;
}

// the last iteration's residual cube, dispersed frame, into R [N] on the
// session stream (ic_get_residual, ic_get_residual_quantised)
static hipError_t launch_residual_cube(Session *s, float *R)
{
    const ic_params &p = s->p;
    int pr_start = p.pr_start < 0 ? 0 : (p.pr_start > p.nbin ? p.nbin : p.pr_start);
    int pr_end = p.pr_end < 0 ? 0 : (p.pr_end > p.nbin ? p.nbin : p.pr_end);
    if (s->fftded) {   // residual + dededisperse (the inverse rotation) in one pass
        RotateArgs ra = residual_rotate_args(s, pr_start, pr_end);
        ra.out = R;
        return launch_rotate(s->stream, ra);
    }
    return launch_residual(s->stream, s->D, s->raw, s->base0, s->T64, s->amp, s->info, s->shift, p.nsub, s->nchan,
                           p.nbin, s->ldD, s->dtiled, p.pr_on, p.pr_factor, pr_start, pr_end, R, s->grid_cap);
}

int ic_get_residual(void *session, float *out)
{
    Session *s = (Session *)session;
    if (!s || !out) return fail(IC_EINVAL, "null argument");
    if (s->failed) return failed_session();
    if (!s->ran) return fail(IC_ESTATE, "no completed iteration");
    CK(hipSetDevice(s->device));
    const auto bad = [](hipError_t e) { return named_fail("residual", e); };
    Scratch tmp;   // the output cube; freed after the synchronise below
    float *R = nullptr;
    CK(tmp.mem.alloc_exact(&R, s->N));
    CKF(launch_residual_cube(s, R), bad);
    CKF(hipMemcpyAsync(out, R, sizeof(float) * s->N, hipMemcpyDeviceToHost, s->stream), bad);
    CKF(hipStreamSynchronize(s->stream), bad);
    return IC_OK;
}

int ic_get_residual_quantised_async(void *session, int flags, int16_t *q, float *scl, float *offs)
{
    Session *s = (Session *)session;
    if (!s || !q || !scl || !offs) return fail(IC_EINVAL, "null argument");
    if (int rc = check_q_flags(flags)) return rc;
    if (s->failed) return failed_session();
    if (!s->ran) return fail(IC_ESTATE, "no completed iteration");
    CK(hipSetDevice(s->device));
    const ic_params &p = s->p;
    const bool big_endian = (flags & IC_Q_BIG_ENDIAN) != 0;
    // one kernel forms and encodes the rows of the integer-shift residual; the
    // FFT modes (and rows too long for its LDS) rotate / form them into the f32
    // cube R first, which is free between runs (every iteration rewrites it
    // whole before reading it) and is allocated here if the run did not need it
    const bool fused = !s->fftded && p.nbin <= kResidualQMaxBin;
    // the encoded residual's staging: first use, kept until ic_session_destroy
    if (s->mem.ensure(&s->res_q, s->N) != hipSuccess || s->mem.ensure(&s->res_so, 2 * s->P) != hipSuccess ||
        (!fused && s->mem.ensure(&s->R, s->N) != hipSuccess))
        return fail(IC_ENOMEM, "quantised residual staging (%zu bytes) failed",
                    sizeof(int16_t) * s->N + 2 * sizeof(float) * s->P + (fused ? 0 : sizeof(float) * s->N));
    if (!s->dl_stream) CK(hipStreamCreateWithFlags(&s->dl_stream, hipStreamNonBlocking));
    if (!s->enc_ev) CK(hipEventCreateWithFlags(&s->enc_ev, hipEventDisableTiming));
    if (!s->dl_ev) CK(hipEventCreateWithFlags(&s->dl_ev, hipEventDisableTiming));
    // hazard (b): an earlier download may still be reading res_q / res_so; this
    // encode overwrites them only after it (an event wait on the session's
    // stream: one staging, and the host does not block)
    if (s->dl_pending) CK(hipStreamWaitEvent(s->stream, s->dl_ev, 0));
    const auto bad = [](hipError_t e) { return named_fail("quantised residual", e); };
    if (fused) {
        ResidualQArgs a{};
        a.D = s->D;
        a.raw = s->raw;
        a.base = s->base0;
        a.T64 = s->T64;
        a.amp = s->amp;
        a.info = s->info;
        a.shift = s->shift;
        a.nsub = p.nsub;
        a.nchan = s->nchan;
        a.nbin = p.nbin;
        a.ldD = s->ldD;
        a.dtiled = s->dtiled;
        a.pr_on = p.pr_on;
        a.pr_factor = p.pr_factor;
        a.pr_start = p.pr_start < 0 ? 0 : (p.pr_start > p.nbin ? p.nbin : p.pr_start);
        a.pr_end = p.pr_end < 0 ? 0 : (p.pr_end > p.nbin ? p.nbin : p.pr_end);
        a.big_endian = big_endian;
        a.q = s->res_q;
        a.scl = s->res_so;
        a.offs = s->res_so + s->P;
        a.grid_cap = s->grid_cap;
        LAUNCH(s, K_RESIDUAL_Q, launch_residual_q(s->stream, a));
    } else {
        CKF(launch_residual_cube(s, s->R), bad);
        CKF(launch_encode_q(s->stream, s->R, (int)s->P, p.nbin, big_endian, s->res_q, s->res_so, s->res_so + s->P,
                            s->grid_cap), bad);
    }
    CKF(hipEventRecord(s->enc_ev, s->stream), bad);
    s->enc_slot = s->cur;   // hazard (a), closed in async_slot
    // hazard (c): a following ic_run queues behind the encode on the session's
    // stream and touches neither res_q / res_so nor the caller's arrays, so it
    // needs no wait for the copies below
    CKF(hipStreamWaitEvent(s->dl_stream, s->enc_ev, 0), bad);
    CKF(hipMemcpyAsync(q, s->res_q, sizeof(int16_t) * s->N, hipMemcpyDeviceToHost, s->dl_stream), bad);
    CKF(hipMemcpyAsync(scl, s->res_so, sizeof(float) * s->P, hipMemcpyDeviceToHost, s->dl_stream), bad);
    CKF(hipMemcpyAsync(offs, s->res_so + s->P, sizeof(float) * s->P, hipMemcpyDeviceToHost, s->dl_stream), bad);
    CKF(hipEventRecord(s->dl_ev, s->dl_stream), bad);
    s->dl_pending = true;
    return IC_OK;
}

int ic_residual_wait(void *session)
{
    Session *s = (Session *)session;
    if (!s) return fail(IC_EINVAL, "null session");
    if (s->failed) return failed_session();
    if (!s->dl_pending) return IC_OK;
    CK(hipSetDevice(s->device));
    const hipError_t e = poll_event(s, s->dl_ev);
    if (e != hipSuccess) return named_fail("ic_residual_wait", e);
    s->dl_pending = false;
    return IC_OK;
}

// one path: the asynchronous call, then its wait
int ic_get_residual_quantised(void *session, int flags, int16_t *q, float *scl, float *offs)
{
    if (int rc = ic_get_residual_quantised_async(session, flags, q, scl, offs)) return rc;
    return ic_residual_wait(session);
}

int ic_encode_profiles(int device, int nsub, int nchan, int nbin, const float *in, int flags, int16_t *q,
                       float *scl, float *offs)
{
    if (!in || !q || !scl || !offs) return fail(IC_EINVAL, "null argument");
    if (int rc = check_q_flags(flags)) return rc;
    if (nsub <= 0 || nchan <= 0 || nbin <= 0 || (size_t)nsub * nchan > (size_t)INT32_MAX)
        return fail(IC_EINVAL, "bad shape (%d, %d, %d)", nsub, nchan, nbin);
    if (int rc = select_device(device)) return rc;
    const size_t P = (size_t)nsub * nchan, N = P * nbin;
    const auto bad = [](hipError_t e) { return named_fail("ic_encode_profiles", e, true); };
    Scratch sc;
    float *d = nullptr, *dso = nullptr;
    int16_t *dq = nullptr;
    CKF(sc.open_stream(), bad);
    hipStream_t st = sc.stream;
    CKF(sc.mem.alloc_exact(&d, N), bad);
    CKF(sc.mem.alloc_exact(&dq, N), bad);
    CKF(sc.mem.alloc_exact(&dso, P * 2), bad);
    CKF(hipMemcpyAsync(d, in, sizeof(float) * N, hipMemcpyHostToDevice, st), bad);
    CKF(launch_encode_q(st, d, (int)P, nbin, (flags & IC_Q_BIG_ENDIAN) != 0, dq, dso, dso + P), bad);
    CKF(hipMemcpyAsync(q, dq, sizeof(int16_t) * N, hipMemcpyDeviceToHost, st), bad);
    CKF(hipMemcpyAsync(scl, dso, sizeof(float) * P, hipMemcpyDeviceToHost, st), bad);
    CKF(hipMemcpyAsync(offs, dso + P, sizeof(float) * P, hipMemcpyDeviceToHost, st), bad);
    CKF(hipStreamSynchronize(st), bad);
    return IC_OK;
}

int ic_set_delays(void *session, const double *delay_bins)
{
    Session *s = (Session *)session;
    if (!s || !delay_bins) return fail(IC_EINVAL, "null argument");
    if (s->failed) return failed_session();
    if (!s->fftded) return fail(IC_ESTATE, "ic_set_delays on a session with dedisp_mode %d", s->p.dedisp_mode);
    for (int c = 0; c < s->nchan; ++c)
        if (!isfinite(delay_bins[c])) return fail(IC_EINVAL, "delay[%d] is not finite", c);
    CK(hipSetDevice(s->device));
    // the table is built on the device (k_phasor_table), as an attached
    // upload's is: one code path
    if (!s->dly && s->mem.alloc_exact(&s->dly, s->P) != hipSuccess) return fail(IC_ENOMEM, "hipMalloc(delays) failed");
    s->delay2 = nullptr;   // dly holds the channel row from here on
    s->delays_set = false;
    CK(hipMemcpyAsync(s->dly, delay_bins, sizeof(double) * s->nchan, hipMemcpyHostToDevice, s->stream));
    CK(launch_phasor_table(s->stream, s->dly, s->nchan, s->p.nbin, s->ph, s->grid_cap));
    CK(hipStreamSynchronize(s->stream));
    s->delays_set = true;
    return IC_OK;
}

int ic_upload_delays_async(void *session, const double *delay_bins, int per_profile)
{
    Session *s = (Session *)session;
    if (!s || !delay_bins) return fail(IC_EINVAL, "null argument");
    if (s->failed) return failed_session();
    if (!s->fftded)
        return fail(IC_ESTATE, "ic_upload_delays_async on a session with dedisp_mode %d", s->p.dedisp_mode);
    if (per_profile != 0 && per_profile != 1) return fail(IC_EINVAL, "per_profile=%d (0 or 1)", per_profile);
    if (!s->fifo_n) return fail(IC_ESTATE, "ic_upload_delays_async without a pending asynchronous upload");
    const int slot = s->fifo[s->fifo_n - 1];
    if (s->slot_dmode[slot]) return fail(IC_ESTATE, "the newest pending upload already has delays");
    const int nsub = s->p.nsub, nchan = s->nchan;
    const size_t nd = per_profile ? s->P : (size_t)nchan;
    for (size_t k = 0; k < nd; ++k)
        if (!isfinite(delay_bins[k])) return fail(IC_EINVAL, "delay[%zu] is not finite", k);
    // equal rows take the channel table, as in ic_set_delays2
    bool table = !per_profile;
    if (per_profile) {
        table = true;
        for (int sb = 1; sb < nsub && table; ++sb)
            table = memcmp(delay_bins, delay_bins + (size_t)sb * nchan, sizeof(double) * nchan) == 0;
    }
    CK(hipSetDevice(s->device));
    if (!s->slot_dly[slot] && s->mem.alloc_exact(&s->slot_dly[slot], s->P) != hipSuccess)
        return fail(IC_ENOMEM, "hipMalloc(slot delays, %zu bytes) failed", sizeof(double) * s->P);
    if (table && s->mem.ensure(&s->slot_ph[slot], 2 * (size_t)nchan * (s->p.nbin / 2 + 1)) != hipSuccess)
        return fail(IC_ENOMEM, "hipMalloc(slot phasor table, %zu bytes) failed",
                    sizeof(float) * 2 * (size_t)nchan * (s->p.nbin / 2 + 1));
    // behind the upload's copies on the copy stream; the slot's event moves
    // behind the delays' copy and the table kernel, so ic_run waits for both
    CK(hipMemcpyAsync(s->slot_dly[slot], delay_bins, sizeof(double) * (table ? (size_t)nchan : s->P),
                      hipMemcpyHostToDevice, s->copy_stream));
    if (table)
        CK(launch_phasor_table(s->copy_stream, s->slot_dly[slot], nchan, s->p.nbin, s->slot_ph[slot], s->grid_cap));
    CK(hipEventRecord(s->slot_ev[slot], s->copy_stream));
    s->slot_dmode[slot] = table ? 1 : 2;
    return IC_OK;
}

int ic_set_delays2(void *session, const double *delay_bins)
{
    Session *s = (Session *)session;
    if (!s || !delay_bins) return fail(IC_EINVAL, "null argument");
    if (s->failed) return failed_session();
    if (!s->fftded) return fail(IC_ESTATE, "ic_set_delays2 on a session with dedisp_mode %d", s->p.dedisp_mode);
    const int nsub = s->p.nsub, nchan = s->nchan;
    for (size_t k = 0; k < (size_t)nsub * nchan; ++k)
        if (!isfinite(delay_bins[k])) return fail(IC_EINVAL, "delay[%zu] is not finite", k);
    // one delay row for every subint: the channel table (the same phasors)
    bool rows_equal = true;
    for (int sb = 1; sb < nsub && rows_equal; ++sb)
        rows_equal = memcmp(delay_bins, delay_bins + (size_t)sb * nchan, sizeof(double) * nchan) == 0;
    if (rows_equal) return ic_set_delays(session, delay_bins);
    CK(hipSetDevice(s->device));
    if (!s->dly && s->mem.alloc_exact(&s->dly, s->P) != hipSuccess)
        return fail(IC_ENOMEM, "hipMalloc(per-profile delays) failed");
    CK(hipMemcpyAsync(s->dly, delay_bins, sizeof(double) * s->P, hipMemcpyHostToDevice, s->stream));
    CK(hipStreamSynchronize(s->stream));
    s->delay2 = s->dly;
    s->delays_set = true;
    return IC_OK;
}

namespace {
// ic_rotate_profiles(2): per_profile = 0: delay_bins [nchan] (the phasor
// table), 1: [nsub*nchan] (phasors evaluated per profile in the kernel)
int rotate_profiles(int device, int nsub, int nchan, int nbin, const float *in, const double *delay_bins,
                    int per_profile, int sign, float *out, bool any = false)
{
    if (!in || !delay_bins || !out || nsub <= 0 || nchan <= 0) return fail(IC_EINVAL, "bad argument");
    const bool czt = any && czt_supported(nbin);   // ic_rotate_profiles_any at a chirp-z length
    if (!rotate_supported(nbin) && !czt)
        return fail(IC_EINVAL, "fractional dedispersion needs " IC_ROT_NBIN_FMT IC_CZT_NBIN_FMT " (nbin=%d)",
                    IC_ROT_NBIN_ARGS, IC_CZT_NBIN_ARGS, nbin);
    if (sign != 1 && sign != -1) return fail(IC_EINVAL, "sign must be +1 or -1");
    const size_t nd = per_profile ? (size_t)nsub * nchan : (size_t)nchan;
    for (size_t c = 0; c < nd; ++c)
        if (!isfinite(delay_bins[c])) return fail(IC_EINVAL, "delay[%zu] is not finite", c);
    if (int rc = select_device(device)) return rc;
    const size_t N = (size_t)nsub * nchan * nbin;
    const std::vector<float> ph = per_profile ? std::vector<float>(2) : make_phasors(nbin, nchan, delay_bins);
    const std::vector<double2> tw = host_twiddles(nbin), tw2 = p2_twiddles(nbin);   // tw2: the rotation's stage tables
    const std::vector<float> ct = czt ? czt_tables(nbin) : std::vector<float>();
    const auto bad = [](hipError_t e) { return named_fail("ic_rotate_profiles", e); };
    Scratch sc;
    float *d = nullptr, *dph = nullptr, *dct = nullptr;
    double2 *dtw = nullptr, *dtw2 = nullptr;
    double *ddl = nullptr;
    CKF(sc.open_stream(), bad);
    hipStream_t st = sc.stream;
    CKF(sc.mem.alloc_exact(&d, N), bad);
    if (per_profile) {
        CKF(sc.mem.alloc_exact(&ddl, nd), bad);
        CKF(hipMemcpyAsync(ddl, delay_bins, sizeof(double) * nd, hipMemcpyHostToDevice, st), bad);
    }
    CKF(sc.mem.alloc_exact(&dph, ph.size()), bad);
    CKF(sc.mem.alloc_exact(&dtw, tw.size()), bad);
    CKF(hipMemcpyAsync(d, in, sizeof(float) * N, hipMemcpyHostToDevice, st), bad);
    CKF(hipMemcpyAsync(dph, ph.data(), sizeof(float) * ph.size(), hipMemcpyHostToDevice, st), bad);
    CKF(hipMemcpyAsync(dtw, tw.data(), sizeof(double2) * tw.size(), hipMemcpyHostToDevice, st), bad);
    if (!tw2.empty()) {   // a power-of-two nbin; k_rotate_mr reads tw alone
        CKF(sc.mem.alloc_exact(&dtw2, tw2.size()), bad);
        CKF(hipMemcpyAsync(dtw2, tw2.data(), sizeof(double2) * tw2.size(), hipMemcpyHostToDevice, st), bad);
    }
    if (czt) {
        CKF(sc.mem.alloc_exact(&dct, ct.size()), bad);
        CKF(hipMemcpyAsync(dct, ct.data(), sizeof(float) * ct.size(), hipMemcpyHostToDevice, st), bad);
    }
    RotateArgs a{};
    a.czt = dct;
    a.in = d;
    a.ld_in = nbin;
    a.ph = per_profile ? nullptr : dph;
    a.delay2 = ddl;
    a.sign = sign;
    a.tw = dtw;
    a.tw_p2 = dtw2;
    a.nsub = nsub;
    a.nchan = nchan;
    a.nbin = nbin;
    a.out = d;
    a.ldo = nbin;
    CKF(launch_rotate(st, a), bad);
    CKF(hipMemcpyAsync(out, d, sizeof(float) * N, hipMemcpyDeviceToHost, st), bad);
    CKF(hipStreamSynchronize(st), bad);
    return IC_OK;
}
}  // namespace

int ic_rotate_profiles(int device, int nsub, int nchan, int nbin, const float *in, const double *delay_bins,
                       int sign, float *out)
{
    return rotate_profiles(device, nsub, nchan, nbin, in, delay_bins, 0, sign, out);
}

int ic_rotate_profiles2(int device, int nsub, int nchan, int nbin, const float *in, const double *delay_bins,
                        int sign, float *out)
{
    return rotate_profiles(device, nsub, nchan, nbin, in, delay_bins, 1, sign, out);
}

int ic_rotate_profiles_any(int device, int nsub, int nchan, int nbin, const float *in, const double *delay_bins,
                           int per_profile, int sign, float *out)
{
    if (per_profile != 0 && per_profile != 1) return fail(IC_EINVAL, "per_profile must be 0 or 1");
    return rotate_profiles(device, nsub, nchan, nbin, in, delay_bins, per_profile, sign, out, true);
}

int ic_get_bad_fits(void *session, int32_t *per_iter, int n)
{
    Session *s = (Session *)session;
    if (!s || (!per_iter && n > 0)) return fail(IC_EINVAL, "null argument");
    const int m = (int)s->bad_fits.size();
    for (int q = 0; q < m && q < n; ++q) per_iter[q] = s->bad_fits[q];
    return m;
}

int ic_set_fit_tail(void *session, int64_t threshold) { return ic_set_option(session, IC_OPT_FIT_TAIL, threshold); }

// Schedule options (include/iterative_cleaner.h): validated here, read by the
// next ic_run; every setting gives the same bits.
int ic_set_option(void *session, int option, int64_t v)
{
    Session *s = (Session *)session;
    if (!s) return fail(IC_EINVAL, "null session");
    if (s->failed) return fail(IC_ESTATE, "session failed (a host wait timed out); destroy it");
    switch (option) {
    case IC_OPT_FIT_TAIL:
        if (v < 0) return fail(IC_EINVAL, "IC_OPT_FIT_TAIL=%lld < 0", (long long)v);
        s->tail_threshold = (long)v;
        return IC_OK;
    case IC_OPT_DIAG_FORK:
        if (v < 0 || v > 64) return fail(IC_EINVAL, "IC_OPT_DIAG_FORK=%lld outside 0..64", (long long)v);
        if (v > 0 && s->p.fit_mode != IC_FIT_EXACT) return fail(IC_EINVAL, "IC_OPT_DIAG_FORK needs the exact fit");
        s->diag_fork = (int)v;
        return IC_OK;
    case IC_OPT_FORK_DELAY:
        if (v < 0 || v > 8) return fail(IC_EINVAL, "IC_OPT_FORK_DELAY=%lld outside 0..8", (long long)v);
        s->fork_delay = (int)v;
        return IC_OK;
    case IC_OPT_TEMPLATE_INCR:
        if (v != 0 && v != 1) return fail(IC_EINVAL, "IC_OPT_TEMPLATE_INCR=%lld (0 or 1)", (long long)v);
        s->incr = v != 0;
        return IC_OK;
    case IC_OPT_FIT_TILED:
        if (v != 0 && v != 1) return fail(IC_EINVAL, "IC_OPT_FIT_TILED=%lld (0 or 1)", (long long)v);
        if (v && s->fftded && s->p.fit_mode != IC_FIT_EXACT)
            return fail(IC_EINVAL, "IC_OPT_FIT_TILED: the closed-form fit of the FFT mode reads a row-major cube");
        // the fit cube of the last run is in the old layout: its residual
        // (ic_get_residual, the FFT mode's rotation) waits for the next run
        if ((int)v != s->dtiled) s->ran = false;
        s->dtiled = (int)v;
        return IC_OK;
    case IC_OPT_ROWSTAT_WAVES:
        if (v != 0 && v != 4 && v != 8) return fail(IC_EINVAL, "IC_OPT_ROWSTAT_WAVES=%lld (0, 4 or 8)", (long long)v);
        s->ls_knobs.grp_waves = (int)v;
        return IC_OK;
    case IC_OPT_ROWSTAT_MINLEN:
        if (v < 1 || v > 16384) return fail(IC_EINVAL, "IC_OPT_ROWSTAT_MINLEN=%lld outside 1..16384", (long long)v);
        s->ls_knobs.grp_minlen = (int)v;
        return IC_OK;
    case IC_OPT_DIAG_CHAIN:
        if (v != 0 && v != 1) return fail(IC_EINVAL, "IC_OPT_DIAG_CHAIN=%lld (0 or 1)", (long long)v);
        s->diag_chain = v != 0;
        return IC_OK;
    case IC_OPT_SYNC_TIMEOUT_MS:
        if (v < 1) return fail(IC_EINVAL, "IC_OPT_SYNC_TIMEOUT_MS=%lld < 1", (long long)v);
        s->sync_timeout_s = (double)v / 1000.0;
        if (s->comm) s->comm->set_timeout_ms((long long)v);
        return IC_OK;
    case IC_OPT_FIT_SCHEDULE:
        // the persistent lanes schedule (round 4, measured slower than the
        // rounds) was removed in round 5: only the rounds remain
        if (v != IC_FIT_ROUNDS) return fail(IC_EINVAL, "IC_OPT_FIT_SCHEDULE=%lld (only IC_FIT_ROUNDS)", (long long)v);
        return IC_OK;
    case IC_OPT_TAIL_SPLIT:
        if (v < 0 || v > 2) return fail(IC_EINVAL, "IC_OPT_TAIL_SPLIT=%lld (0, 1 or 2)", (long long)v);
        s->tail_split_mode = (int)v;
        return IC_OK;
    case IC_OPT_GRID_CAP:
        if (v < 0 || v > 65536) return fail(IC_EINVAL, "IC_OPT_GRID_CAP=%lld outside 0..65536", (long long)v);
        s->grid_cap = (int)v;
        return IC_OK;
    case IC_OPT_ROT_STATS:
        if (v != 0 && v != 1) return fail(IC_EINVAL, "IC_OPT_ROT_STATS=%lld (0 or 1)", (long long)v);
        s->rot_stats = v != 0;
        return IC_OK;
    default:
        return fail(IC_EINVAL, "unknown option %d", option);
    }
}

int ic_get_option(void *session, int option, int64_t *out)
{
    Session *s = (Session *)session;
    if (!s || !out) return fail(IC_EINVAL, "null argument");
    switch (option) {
    case IC_OPT_FIT_TAIL: *out = s->tail_threshold; return IC_OK;
    case IC_OPT_DIAG_FORK: *out = s->diag_fork; return IC_OK;
    case IC_OPT_FORK_DELAY: *out = s->fork_delay; return IC_OK;
    case IC_OPT_TEMPLATE_INCR: *out = s->incr ? 1 : 0; return IC_OK;
    case IC_OPT_FIT_TILED: *out = s->dtiled; return IC_OK;
    case IC_OPT_ROWSTAT_WAVES: *out = s->ls_knobs.grp_waves; return IC_OK;
    case IC_OPT_ROWSTAT_MINLEN: *out = s->ls_knobs.grp_minlen; return IC_OK;
    case IC_OPT_DIAG_CHAIN: *out = s->diag_chain ? 1 : 0; return IC_OK;
    case IC_OPT_SYNC_TIMEOUT_MS: *out = (int64_t)(s->sync_timeout_s * 1000.0 + 0.5); return IC_OK;
    case IC_OPT_FIT_SCHEDULE: *out = IC_FIT_ROUNDS; return IC_OK;
    case IC_OPT_TAIL_SPLIT: *out = s->tail_split_mode; return IC_OK;
    case IC_OPT_ROT_STATS: *out = s->rot_stats ? 1 : 0; return IC_OK;
    case IC_OPT_GRID_CAP: *out = s->grid_cap; return IC_OK;
    default: return fail(IC_EINVAL, "unknown option %d", option);
    }
}

// the ranges of ic_set_detrend / ic_comprehensive_stats_detrend; 0 or the message
static const char *detrend_range(int chan_order, int subint_order, int rounds, double clip)
{
    if (chan_order < 0 || chan_order > 3 || subint_order < 0 || subint_order > 3) return "orders outside 0..3";
    if (rounds < 1 || rounds > 8) return "rounds outside 1..8";
    if (!(std::isfinite(clip) && clip > 0.0)) return "clip must be finite and > 0";
    return nullptr;
}

int ic_set_detrend(void *session, int chan_order, int subint_order, int rounds, double clip)
{
    Session *s = (Session *)session;
    if (!s) return fail(IC_EINVAL, "null session");
    if (s->failed) return failed_session();
    if (const char *e = detrend_range(chan_order, subint_order, rounds, clip))
        return fail(IC_EINVAL, "ic_set_detrend(%d, %d, %d, %g): %s", chan_order, subint_order, rounds, clip, e);
    if ((s->comm || s->world > 1) && !s->sh_dt)
        return fail(IC_EINVAL, "ic_set_detrend on a channel shard: detrended rows across shards are not supported "
                               "(unless every rank opts in first: ic_shard_enable_detrend)");
    s->dt_chan = chan_order;
    s->dt_sub = subint_order;
    s->dt_rounds = rounds;
    s->dt_clip = clip;
    s->trends_ran = false;
    return IC_OK;
}

int ic_get_trends(void *session, double *chan_coef, double *subint_coef)
{
    Session *s = (Session *)session;
    if (!s) return fail(IC_EINVAL, "null session");
    if (s->failed) return failed_session();
    if (!(s->dt_chan > 0 || s->dt_sub > 0)) return fail(IC_ESTATE, "detrending is off (ic_set_detrend)");
    if (!s->ran || !s->trends_ran) return fail(IC_ESTATE, "no completed detrended iteration");
    if (s->pw_on && (s->pw_cs.size() > 1 || s->pw_ss.size() > 1))
        return fail(IC_ESTATE, "a direction has more than one piece: ic_get_trends_pieces");
    // one piece each: the piecewise arrays have this layout
    const double *trend = s->pw_on ? s->pw_trend : s->trend;
    const size_t nc = (size_t)16 * s->nchan, ns = (size_t)16 * s->p.nsub;
    if (chan_coef) CK(hipMemcpyAsync(chan_coef, trend, sizeof(double) * nc, hipMemcpyDeviceToHost, s->stream));
    if (subint_coef)
        CK(hipMemcpyAsync(subint_coef, trend + nc, sizeof(double) * ns, hipMemcpyDeviceToHost, s->stream));
    CK(hipStreamSynchronize(s->stream));
    return IC_OK;
}

int ic_set_detrend_pieces(void *session, int chan_npieces, const int32_t *chan_starts, int subint_npieces,
                          const int32_t *subint_starts)
{
    Session *s = (Session *)session;
    if (!s) return fail(IC_EINVAL, "null session");
    if (s->failed) return failed_session();
    if ((s->comm || s->world > 1) && !s->sh_dt)
        return fail(IC_EINVAL, "ic_set_detrend_pieces on a channel shard: detrended rows across shards are not supported "
                               "(unless every rank opts in first: ic_shard_enable_detrend)");
    if (const char *e = pieces_range(chan_npieces, chan_starts, s->p.nsub))
        return fail(IC_EINVAL, "ic_set_detrend_pieces, channel lines (%d entries): %s", s->p.nsub, e);
    // a subint line is the archive's (p.nchan == nchan unless this is a shard)
    if (const char *e = pieces_range(subint_npieces, subint_starts, s->p.nchan))
        return fail(IC_EINVAL, "ic_set_detrend_pieces, subint lines (%d entries): %s", s->p.nchan, e);
    s->pw_on = chan_npieces > 0 || subint_npieces > 0;
    s->pw_cs.assign(1, 0);
    s->pw_ss.assign(1, 0);
    if (chan_npieces > 0) s->pw_cs.assign(chan_starts, chan_starts + chan_npieces);
    if (subint_npieces > 0) s->pw_ss.assign(subint_starts, subint_starts + subint_npieces);
    // the tables and coefficient arrays of the pieces before: a run ends
    // synchronised, so nothing reads them; the next piecewise run allocates anew
    s->mem.release(s->pw_starts);
    s->mem.release(s->pw_piece);
    s->mem.release(s->pw_trend);
    if (s->comm) {   // a shard's slots were sized for the pieces before
        s->comm->release(s->xt_send);
        s->comm->release(s->xt_recv);
        s->xt_send = s->xt_recv = nullptr;
        s->xt_ms = 0;
    }
    s->trends_ran = false;
    return IC_OK;
}

int ic_shard_enable_detrend(void *session)
{
    Session *s = (Session *)session;
    if (!s) return fail(IC_EINVAL, "null session");
    if (s->failed) return failed_session();
    if (s->comm || s->world > 1) s->sh_dt = true;
    return IC_OK;
}

int ic_get_trends_pieces(void *session, double *chan_coef, double *subint_coef)
{
    Session *s = (Session *)session;
    if (!s) return fail(IC_EINVAL, "null session");
    if (s->failed) return failed_session();
    if (!(s->dt_chan > 0 || s->dt_sub > 0)) return fail(IC_ESTATE, "detrending is off (ic_set_detrend)");
    if (!s->pw_on) return fail(IC_ESTATE, "no pieces are set (ic_set_detrend_pieces)");
    if (!s->ran || !s->trends_ran) return fail(IC_ESTATE, "no completed detrended iteration");
    const size_t nc = (size_t)16 * s->nchan * s->pw_cs.size(), ns = (size_t)16 * s->p.nsub * s->pw_ss.size();
    if (chan_coef) CK(hipMemcpyAsync(chan_coef, s->pw_trend, sizeof(double) * nc, hipMemcpyDeviceToHost, s->stream));
    if (subint_coef)
        CK(hipMemcpyAsync(subint_coef, s->pw_trend + nc, sizeof(double) * ns, hipMemcpyDeviceToHost, s->stream));
    CK(hipStreamSynchronize(s->stream));
    return IC_OK;
}

int ic_get_run_stats(void *session, ic_run_stats *out)
{
    Session *s = (Session *)session;
    if (!s || !out) return fail(IC_EINVAL, "null argument");
    *out = s->stats;
    return IC_OK;
}

int ic_get_template(void *session, float *T)
{
    Session *s = (Session *)session;
    if (!s || !T) return fail(IC_EINVAL, "null argument");
    if (s->failed) return failed_session();
    if (!s->ran) return fail(IC_ESTATE, "no completed iteration");
    CK(hipMemcpyAsync(T, s->T, sizeof(float) * s->p.nbin, hipMemcpyDeviceToHost, s->stream));
    CK(hipStreamSynchronize(s->stream));
    return IC_OK;
}

static_assert(IC_ALIGN_NONE == kAlignNone && IC_ALIGN_INT == kAlignInt && IC_ALIGN_FRAC == kAlignFrac,
              "the public alignment modes are the kernels'");

// the argument rules ic_set_std_template and ic_align_template share; 0 or the
// failed call's return code
static int std_args(const char *name, const float *S, int nbin, int align)
{
    if (align != IC_ALIGN_NONE && align != IC_ALIGN_INT && align != IC_ALIGN_FRAC)
        return fail(IC_EINVAL, "%s: align=%d (IC_ALIGN_NONE, IC_ALIGN_INT or IC_ALIGN_FRAC)", name, align);
    if (const char *e = std_check(S, nbin)) return fail(IC_EINVAL, "%s: the standard has %s", name, e);
    if (align == IC_ALIGN_FRAC && !rotate_supported(nbin))
        return fail(IC_EINVAL, "%s: IC_ALIGN_FRAC needs " IC_ROT_NBIN_FMT " (nbin=%d); use IC_ALIGN_INT", name,
                    IC_ROT_NBIN_ARGS, nbin);
    if (std_ccf_lds_bytes(nbin) > kLdsBlockMax)
        return fail(IC_EINVAL, "%s: nbin=%d needs %zu bytes of LDS for the cross-correlation (> 160 KiB)", name, nbin,
                    std_ccf_lds_bytes(nbin));
    return IC_OK;
}

int ic_set_std_template(void *session, const float *T, int nbin, int align)
{
    Session *s = (Session *)session;
    if (!s) return fail(IC_EINVAL, "null session");
    if (s->failed) return failed_session();
    if (!T) {   // back to the iterative template
        s->std_on = false;
        s->std_ran = false;
        return IC_OK;
    }
    if (nbin != s->p.nbin)
        return fail(IC_EINVAL, "ic_set_std_template: the standard has %d bins, the session %d (a standard of another "
                               "length is not rebinned)", nbin, s->p.nbin);
    if (int rc = std_args("ic_set_std_template", T, nbin, align)) return rc;
    CK(hipSetDevice(s->device));
    if (s->mem.ensure(&s->std_S, (size_t)nbin) != hipSuccess || s->mem.ensure(&s->std_rot, (size_t)nbin) != hipSuccess ||
        s->mem.ensure(&s->std_c, (size_t)nbin) != hipSuccess || s->mem.ensure(&s->std_rec, 1) != hipSuccess)
        return fail(IC_ENOMEM, "hipMalloc(standard template, %d bins) failed", nbin);
    // a run ends synchronised, so nothing reads the standard set before
    s->std_on = false;
    CK(hipMemcpyAsync(s->std_S, T, sizeof(float) * nbin, hipMemcpyHostToDevice, s->stream));
    CK(hipMemsetAsync(s->std_rec, 0, sizeof(StdAlignRec), s->stream));
    CK(hipStreamSynchronize(s->stream));
    s->std_mean = std_mean_of(T, nbin);
    uint32_t h = 2166136261u;   // FNV-1a over the samples' bytes, then the mode
    const unsigned char *b = (const unsigned char *)T;
    for (size_t q = 0; q < sizeof(float) * (size_t)nbin; ++q) h = (h ^ b[q]) * 16777619u;
    h = (h ^ (uint32_t)align) * 16777619u;
    s->std_hash = (h ^ (h >> 30)) & 0x3fffffffu;
    s->std_mode = align;
    s->std_on = true;
    s->std_ran = false;
    return IC_OK;
}

int ic_get_std_alignment(void *session, int32_t *aligned, int32_t *lag, double *shift)
{
    Session *s = (Session *)session;
    if (!s) return fail(IC_EINVAL, "null session");
    if (s->failed) return failed_session();
    if (!s->std_on) return fail(IC_ESTATE, "no standard template is set (ic_set_std_template)");
    if (!s->ran || !s->std_ran) return fail(IC_ESTATE, "no completed run with the standard template");
    CK(hipSetDevice(s->device));
    StdAlignRec r;
    CK(hipMemcpyAsync(&r, s->std_rec, sizeof r, hipMemcpyDeviceToHost, s->stream));
    CK(hipStreamSynchronize(s->stream));
    if (aligned) *aligned = r.aligned;
    if (lag) *lag = r.lag;
    if (shift) *shift = r.shift;
    return IC_OK;
}

int ic_align_template(int device, int nbin, const float *S, const float *A, int align, float *out, int32_t *aligned,
                      int32_t *lag, double *shift)
{
    if (!S || !A || !out) return fail(IC_EINVAL, "null argument");
    if (int rc = std_args("ic_align_template", S, nbin, align)) return rc;
    if (int rc = select_device(device)) return rc;
    const auto bad = [](hipError_t e) { return named_fail("ic_align_template", e, true); };
    const int ldD = ((nbin + kFitTile - 1) / kFitTile) * kFitTile;
    Scratch sc;
    float *dS = nullptr, *dA = nullptr, *dR = nullptr, *dT = nullptr;
    double *dc = nullptr, *dT64 = nullptr, *dT2 = nullptr;
    double2 *dtw = nullptr, *dtw2 = nullptr;
    StdAlignRec *drec = nullptr;
    CKF(sc.open_stream(), bad);
    hipStream_t st = sc.stream;
    CKF(sc.mem.alloc(&dS, (size_t)nbin), bad);
    CKF(sc.mem.alloc(&dA, (size_t)nbin), bad);
    CKF(sc.mem.alloc(&dR, (size_t)nbin), bad);
    CKF(sc.mem.alloc(&dT, (size_t)nbin), bad);
    CKF(sc.mem.alloc(&dc, (size_t)nbin), bad);
    CKF(sc.mem.alloc(&dT64, (size_t)ldD), bad);
    CKF(sc.mem.alloc(&dT2, (size_t)2 * nbin), bad);
    CKF(sc.mem.alloc(&drec, 1), bad);
    CKF(hipMemcpyAsync(dS, S, sizeof(float) * nbin, hipMemcpyHostToDevice, st), bad);
    CKF(hipMemcpyAsync(dA, A, sizeof(float) * nbin, hipMemcpyHostToDevice, st), bad);
    CKF(hipMemsetAsync(drec, 0, sizeof(StdAlignRec), st), bad);
    if (align != IC_ALIGN_NONE) {
        CKF(launch_std_ccf(st, dS, dA, nbin, std_mean_of(S, nbin), dc), bad);
        CKF(launch_std_peak(st, dc, nbin, drec), bad);
    }
    std::vector<double2> tw, tw2;   // alive until the stream is synchronised
    if (align == IC_ALIGN_FRAC) {
        tw = host_twiddles(nbin);
        tw2 = p2_twiddles(nbin);   // empty at a mixed-radix nbin: k_rotate_mr reads tw alone
        CKF(sc.mem.alloc_exact(&dtw, tw.size()), bad);
        CKF(hipMemcpyAsync(dtw, tw.data(), sizeof(double2) * tw.size(), hipMemcpyHostToDevice, st), bad);
        if (!tw2.empty()) {
            CKF(sc.mem.alloc_exact(&dtw2, tw2.size()), bad);
            CKF(hipMemcpyAsync(dtw2, tw2.data(), sizeof(double2) * tw2.size(), hipMemcpyHostToDevice, st), bad);
        }
        CKF(launch_rotate(st, std_rotate_args(dS, drec, nbin, dtw, dtw2, dR, 0)), bad);
    }
    CKF(launch_std_install(st, dS, dR, drec, align, nbin, ldD, dT, dT64, dT2), bad);
    StdAlignRec r;
    CKF(hipMemcpyAsync(out, dT, sizeof(float) * nbin, hipMemcpyDeviceToHost, st), bad);
    CKF(hipMemcpyAsync(&r, drec, sizeof r, hipMemcpyDeviceToHost, st), bad);
    CKF(hipStreamSynchronize(st), bad);
    if (aligned) *aligned = r.aligned;
    if (lag) *lag = r.lag;
    if (shift) *shift = r.shift;
    return IC_OK;
}

int ic_set_hotbins(void *session, double threshold, int on_start, int on_end, int rounds)
{
    Session *s = (Session *)session;
    if (!s) return fail(IC_EINVAL, "null session");
    if (s->failed) return failed_session();
    if (threshold <= 0.0) {   // off: the session launches what it did before
        s->hb_on = false;
        return IC_OK;
    }
    if (const char *e = hotbins_range(s->p.nbin, threshold, on_start, on_end, rounds, hot_widen(s)))
        return fail(IC_EINVAL, "ic_set_hotbins(%g, %d, %d, %d) at nbin=%d: %s", threshold, on_start, on_end, rounds,
                    s->p.nbin, e);
    // "the uploads consumed from here on": an upload that a run has already
    // read while the option was off keeps its cube as it is
    if (!s->hb_on && s->ran) s->hb_done = true;
    s->hb_on = true;
    s->hb_thr = threshold;
    s->hb_start = on_start;
    s->hb_end = on_end;
    s->hb_rounds = rounds;
    return IC_OK;
}

static int hotbins_state(const Session *s, const char *name)
{
    if (!s->hb_on) return fail(IC_ESTATE, "%s: hot-bin repair is off (ic_set_hotbins)", name);
    if (!s->hb_have) return fail(IC_ESTATE, "%s: no run has consumed an upload with hot-bin repair on", name);
    return IC_OK;
}

int ic_get_hotbins(void *session, int32_t *count, int64_t *total)
{
    Session *s = (Session *)session;
    if (!s) return fail(IC_EINVAL, "null session");
    if (s->failed) return failed_session();
    if (int rc = hotbins_state(s, "ic_get_hotbins")) return rc;
    CK(hipSetDevice(s->device));
    if (count) CK(hipMemcpyAsync(count, s->hb_count, sizeof(int32_t) * s->P, hipMemcpyDeviceToHost, s->stream));
    if (total) CK(hipMemcpyAsync(total, s->hb_total, sizeof(int64_t), hipMemcpyDeviceToHost, s->stream));
    CK(hipStreamSynchronize(s->stream));
    return IC_OK;
}

int ic_get_hotbin_list(void *session, int32_t *bins, int64_t cap)
{
    Session *s = (Session *)session;
    if (!s) return fail(IC_EINVAL, "null session");
    if (s->failed) return failed_session();
    if (int rc = hotbins_state(s, "ic_get_hotbin_list")) return rc;
    CK(hipSetDevice(s->device));
    int64_t total = 0;
    CK(hipMemcpyAsync(&total, s->hb_total, sizeof(int64_t), hipMemcpyDeviceToHost, s->stream));
    CK(hipStreamSynchronize(s->stream));
    if (cap < total) return fail(IC_EINVAL, "ic_get_hotbin_list: cap=%lld below the list's %lld entries",
                                 (long long)cap, (long long)total);
    if (total == 0) return IC_OK;
    if (!bins) return fail(IC_EINVAL, "ic_get_hotbin_list: null bins");
    const auto bad = [](hipError_t e) { return named_fail("ic_get_hotbin_list", e, true); };
    Scratch tmp;
    int32_t *d = nullptr;
    CKF(tmp.mem.alloc_exact(&d, (size_t)total), bad);
    CKF(launch_hotbin_fill(s->stream, s->hb_count, s->hb_mask, s->hb_offs, (long)s->P, s->p.nbin, d, total,
                           s->grid_cap), bad);
    CKF(hipMemcpyAsync(bins, d, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, s->stream), bad);
    CKF(hipStreamSynchronize(s->stream), bad);   // before tmp frees d
    return IC_OK;
}

int ic_hotbins_profiles(int device, int nprof, int nbin, const float *in, const float *w, const int32_t *offsets,
                        int widen, double threshold, int on_start, int on_end, int rounds, float *out,
                        int32_t *count, int32_t *bins, int64_t cap, int64_t *total)
{
    if (!in || !w || !count || !total) return fail(IC_EINVAL, "null argument");
    if (nprof <= 0 || nbin <= 0) return fail(IC_EINVAL, "bad shape nprof=%d nbin=%d", nprof, nbin);
    if (widen != 0 && widen != 1) return fail(IC_EINVAL, "widen=%d (0 or 1)", widen);
    if (cap < 0 || (bins == nullptr && cap != 0)) return fail(IC_EINVAL, "cap=%lld with%s bins", (long long)cap,
                                                              bins ? "" : " null");
    if (const char *e = hotbins_range(nbin, threshold, on_start, on_end, rounds, widen != 0))
        return fail(IC_EINVAL, "ic_hotbins_profiles(%g, %d, %d, %d) at nbin=%d: %s", threshold, on_start, on_end,
                    rounds, nbin, e);
    if (int rc = select_device(device)) return rc;
    const size_t P = (size_t)nprof, N = P * nbin, words = (size_t)hot_mask_words(nbin);
    const auto bad = [](hipError_t e) { return named_fail("ic_hotbins_profiles", e, true); };
    Scratch sc;
    CKF(sc.open_stream(), bad);
    hipStream_t st = sc.stream;
    HotBinArgs a{};
    float *dw = nullptr;
    int32_t *doff = nullptr, *dbins = nullptr;
    int64_t *doffs = nullptr, *dtotal = nullptr;
    CKF(sc.mem.alloc_exact(&a.cube, N), bad);
    CKF(sc.mem.alloc_exact(&dw, P), bad);
    CKF(sc.mem.alloc_exact(&a.count, P), bad);
    CKF(sc.mem.alloc_exact(&a.mask, P * words), bad);
    CKF(sc.mem.alloc_exact(&doffs, P), bad);
    CKF(sc.mem.alloc_exact(&dtotal, 1 + hotbin_scan_parts((long)P)), bad);
    CKF(hipMemcpyAsync(a.cube, in, sizeof(float) * N, hipMemcpyHostToDevice, st), bad);
    CKF(hipMemcpyAsync(dw, w, sizeof(float) * P, hipMemcpyHostToDevice, st), bad);
    if (offsets) {
        CKF(sc.mem.alloc_exact(&doff, P), bad);
        CKF(hipMemcpyAsync(doff, offsets, sizeof(int32_t) * P, hipMemcpyHostToDevice, st), bad);
    }
    a.w0 = dw;
    a.off32 = doff;
    a.per_profile = 1;
    a.P = (long)P;
    a.nchan = 1;
    a.nbin = nbin;
    hot_window(nbin, on_start, on_end, widen != 0, &a.win_start, &a.win_len);
    a.threshold = threshold;
    a.rounds = rounds;
    CKF(launch_hotbins(st, a), bad);
    CKF(launch_hotbin_scan(st, a.count, (long)P, dtotal + 1, doffs, dtotal), bad);
    if (out) CKF(hipMemcpyAsync(out, a.cube, sizeof(float) * N, hipMemcpyDeviceToHost, st), bad);
    CKF(hipMemcpyAsync(count, a.count, sizeof(int32_t) * P, hipMemcpyDeviceToHost, st), bad);
    CKF(hipMemcpyAsync(total, dtotal, sizeof(int64_t), hipMemcpyDeviceToHost, st), bad);
    CKF(hipStreamSynchronize(st), bad);
    if (!bins) return IC_OK;
    if (cap < *total) return fail(IC_EINVAL, "ic_hotbins_profiles: cap=%lld below the list's %lld entries",
                                  (long long)cap, (long long)*total);
    if (*total == 0) return IC_OK;
    CKF(sc.mem.alloc_exact(&dbins, (size_t)*total), bad);
    CKF(launch_hotbin_fill(st, a.count, a.mask, doffs, (long)P, nbin, dbins, *total), bad);
    CKF(hipMemcpyAsync(bins, dbins, sizeof(int32_t) * (size_t)*total, hipMemcpyDeviceToHost, st), bad);
    CKF(hipStreamSynchronize(st), bad);
    return IC_OK;
}

int ic_get_dynspec(void *session, double *amp, double *err, double *base)
{
    Session *s = (Session *)session;
    if (!s) return fail(IC_EINVAL, "null session");
    if (s->failed) return failed_session();
    if (!s->ran) return fail(IC_ESTATE, "ic_get_dynspec: no completed iteration");
    const int nbin = s->p.nbin;
    if (nbin < kDynMinBin) return fail(IC_EINVAL, "ic_get_dynspec: nbin=%d below %d", nbin, kDynMinBin);
    CK(hipSetDevice(s->device));
    if (s->mem.ensure(&s->ds_tt, (size_t)nbin + 2) != hipSuccess || s->mem.ensure(&s->ds_out, 3 * s->P) != hipSuccess)
        return fail(IC_ENOMEM, "hipMalloc(dynamic spectrum: %zu bytes) failed", 8 * ((size_t)nbin + 2 + 3 * s->P));
    // the cube the last run consumed, dedispersed: the rotated view rot(raw)
    // that prepare() left (an input stored dedispersed: its copy), or raw
    // gathered by the integer shifts
    DynspecArgs a{};
    a.x = s->fftded ? s->dr : s->raw;
    a.shift = s->fftded ? nullptr : s->shift;
    a.w = s->W;
    a.tt = s->ds_tt;
    a.P = (long)s->P;
    a.nchan = s->nchan;
    a.nbin = nbin;
    a.amp = s->ds_out;
    a.err = s->ds_out + s->P;
    a.base = s->ds_out + 2 * s->P;
    a.grid_cap = s->grid_cap;
    CK(launch_dynspec_prep(s->stream, s->T, nbin, s->ds_tt));
    LAUNCH(s, K_DYNSPEC, launch_dynspec(s->stream, a));
    double *const host[3] = {amp, err, base};
    for (int q = 0; q < 3; ++q)
        if (host[q])
            CK(hipMemcpyAsync(host[q], s->ds_out + (size_t)q * s->P, sizeof(double) * s->P, hipMemcpyDeviceToHost,
                              s->stream));
    CK(hipStreamSynchronize(s->stream));
    return IC_OK;
}

int ic_dynspec_profiles(int device, int nprof, int nbin, const float *T, const float *profiles, const float *w,
                        double *amp, double *err, double *base)
{
    if (!T || !profiles || !w) return fail(IC_EINVAL, "null argument");
    if (nprof <= 0) return fail(IC_EINVAL, "bad shape nprof=%d nbin=%d", nprof, nbin);
    if (nbin < kDynMinBin || nbin > 32768)
        return fail(IC_EINVAL, "ic_dynspec_profiles: nbin=%d outside %d..32768", nbin, kDynMinBin);
    if (int rc = select_device(device)) return rc;
    const size_t P = (size_t)nprof, N = P * nbin;
    const auto bad = [](hipError_t e) { return named_fail("ic_dynspec_profiles", e, true); };
    Scratch sc;
    CKF(sc.open_stream(), bad);
    hipStream_t st = sc.stream;
    float *dT = nullptr, *dx = nullptr, *dw = nullptr;
    double *dtt = nullptr, *dout = nullptr;
    CKF(sc.mem.alloc(&dT, (size_t)nbin), bad);
    CKF(sc.mem.alloc_exact(&dx, N), bad);
    CKF(sc.mem.alloc_exact(&dw, P), bad);
    CKF(sc.mem.alloc(&dtt, (size_t)nbin + 2), bad);
    CKF(sc.mem.alloc(&dout, 3 * P), bad);
    CKF(hipMemcpyAsync(dT, T, sizeof(float) * nbin, hipMemcpyHostToDevice, st), bad);
    CKF(hipMemcpyAsync(dx, profiles, sizeof(float) * N, hipMemcpyHostToDevice, st), bad);
    CKF(hipMemcpyAsync(dw, w, sizeof(float) * P, hipMemcpyHostToDevice, st), bad);
    DynspecArgs a{};
    a.x = dx;
    a.w = dw;
    a.tt = dtt;
    a.P = (long)P;
    a.nchan = 1;
    a.nbin = nbin;
    a.amp = dout;
    a.err = dout + P;
    a.base = dout + 2 * P;
    CKF(launch_dynspec_prep(st, dT, nbin, dtt), bad);
    CKF(launch_dynspec(st, a), bad);
    double *const host[3] = {amp, err, base};
    for (int q = 0; q < 3; ++q)
        if (host[q]) CKF(hipMemcpyAsync(host[q], dout + (size_t)q * P, sizeof(double) * P, hipMemcpyDeviceToHost, st), bad);
    CKF(hipStreamSynchronize(st), bad);
    return IC_OK;
}

int ic_get_fit(void *session, double *amp, int32_t *info)
{
    Session *s = (Session *)session;
    if (!s) return fail(IC_EINVAL, "null argument");
    if (s->failed) return failed_session();
    if (!s->ran) return fail(IC_ESTATE, "no completed iteration");
    if (amp) CK(hipMemcpyAsync(amp, s->amp, sizeof(double) * s->P, hipMemcpyDeviceToHost, s->stream));
    if (info) CK(hipMemcpyAsync(info, s->info, sizeof(int32_t) * s->P, hipMemcpyDeviceToHost, s->stream));
    CK(hipStreamSynchronize(s->stream));
    return IC_OK;
}

int ic_get_diagnostics_f64(void *session, double *std_o, double *mean_o, double *ptp_o, double *fftmax_o)
{
    Session *s = (Session *)session;
    if (!s) return fail(IC_EINVAL, "null argument");
    if (s->failed) return failed_session();
    if (!s->ran) return fail(IC_ESTATE, "no completed iteration");
    if (std_o) CK(hipMemcpyAsync(std_o, s->std_, sizeof(double) * s->P, hipMemcpyDeviceToHost, s->stream));
    if (mean_o) CK(hipMemcpyAsync(mean_o, s->mean, sizeof(double) * s->P, hipMemcpyDeviceToHost, s->stream));
    if (ptp_o) CK(hipMemcpyAsync(ptp_o, s->ptp, sizeof(double) * s->P, hipMemcpyDeviceToHost, s->stream));
    if (fftmax_o) CK(hipMemcpyAsync(fftmax_o, s->fft, sizeof(double) * s->P, hipMemcpyDeviceToHost, s->stream));
    CK(hipStreamSynchronize(s->stream));
    return IC_OK;
}

int ic_get_diagnostics(void *session, double *std_o, double *mean_o, float *ptp_o, double *fftmax_o)
{
    Session *s = (Session *)session;
    if (!s) return fail(IC_EINVAL, "null argument");
    std::vector<double> ptp(ptp_o ? s->P : 0);
    if (int rc = ic_get_diagnostics_f64(session, std_o, mean_o, ptp_o ? ptp.data() : nullptr, fftmax_o)) return rc;
    for (size_t k = 0; k < ptp.size(); ++k) ptp_o[k] = (float)ptp[k];   // exact unless data_f64
    return IC_OK;
}

// comprehensive_stats alone (iterative_cleaner.py:181-226 on the data of
// :111-117): one-shot device buffers, the diagnostics kernel in DIAG_STATS mode,
// the line medians and the combine of one "iteration" (weights/history unused).
int ic_comprehensive_stats(int device, int nsub, int nchan, int nbin, const float *data, const float *weights,
                           double chanthresh, double subintthresh, double *test_out, double *std_o, double *mean_o,
                           float *ptp_o, double *fftmax_o)
{
    return ic_comprehensive_stats_rowstat(device, nsub, nchan, nbin, data, weights, chanthresh, subintthresh,
                                          test_out, std_o, mean_o, ptp_o, fftmax_o, 8, 1024);
}

// the one-shot statistics; dt (optional): detrended (k_linetrend, k_combine_dt),
// its coefficient pointers host outputs (may be null); pieces (optional, with
// dt): checked starts of both directions, the piecewise kernels and coefficient
// layout.  ptp goes to ptp_o (f32) or ptp64_o.
struct PieceSpec {
    std::vector<int32_t> cs, ss;
};
static int stats_oneshot(int device, int nsub, int nchan, int nbin, const float *data, const float *weights,
                         double chanthresh, double subintthresh, double *test_out, double *std_o, double *mean_o,
                         float *ptp_o, double *ptp64_o, double *fftmax_o, int rowstat_waves, int rowstat_minlen,
                         int data_f64, const TrendArgs *trend, const PieceSpec *pieces = nullptr);

int ic_comprehensive_stats_rowstat(int device, int nsub, int nchan, int nbin, const float *data,
                                   const float *weights, double chanthresh, double subintthresh, double *test_out,
                                   double *std_o, double *mean_o, float *ptp_o, double *fftmax_o, int rowstat_waves,
                                   int rowstat_minlen)
{
    return stats_oneshot(device, nsub, nchan, nbin, data, weights, chanthresh, subintthresh, test_out, std_o, mean_o,
                         ptp_o, nullptr, fftmax_o, rowstat_waves, rowstat_minlen, 0, nullptr);
}

int ic_comprehensive_stats_detrend(int device, int nsub, int nchan, int nbin, const float *data, const float *weights,
                                   double chanthresh, double subintthresh, double *test_out, double *std_o,
                                   double *mean_o, double *ptp_o, double *fftmax_o, int data_f64, int chan_order,
                                   int subint_order, int rounds, double clip, double *chan_coef, double *subint_coef)
{
    if (data_f64 != 0 && data_f64 != 1) return fail(IC_EINVAL, "data_f64=%d (0 or 1)", data_f64);
    if (const char *e = detrend_range(chan_order, subint_order, rounds, clip))
        return fail(IC_EINVAL, "ic_comprehensive_stats_detrend(%d, %d, %d, %g): %s", chan_order, subint_order, rounds,
                    clip, e);
    const TrendArgs dt{chan_order, subint_order, rounds, clip, chan_coef, subint_coef};
    return stats_oneshot(device, nsub, nchan, nbin, data, weights, chanthresh, subintthresh, test_out, std_o, mean_o,
                         nullptr, ptp_o, fftmax_o, 8, 1024, data_f64, &dt);
}

int ic_comprehensive_stats_detrend_pieces(int device, int nsub, int nchan, int nbin, const float *data,
                                          const float *weights, double chanthresh, double subintthresh,
                                          double *test_out, double *std_o, double *mean_o, double *ptp_o,
                                          double *fftmax_o, int data_f64, int chan_order, int subint_order, int rounds,
                                          double clip, double *chan_coef, double *subint_coef, int chan_npieces,
                                          const int32_t *chan_starts, int subint_npieces, const int32_t *subint_starts)
{
    if (data_f64 != 0 && data_f64 != 1) return fail(IC_EINVAL, "data_f64=%d (0 or 1)", data_f64);
    if (const char *e = detrend_range(chan_order, subint_order, rounds, clip))
        return fail(IC_EINVAL, "ic_comprehensive_stats_detrend_pieces(%d, %d, %d, %g): %s", chan_order, subint_order,
                    rounds, clip, e);
    if (const char *e = pieces_range(chan_npieces, chan_starts, nsub))
        return fail(IC_EINVAL, "ic_comprehensive_stats_detrend_pieces, channel lines (%d entries): %s", nsub, e);
    if (const char *e = pieces_range(subint_npieces, subint_starts, nchan))
        return fail(IC_EINVAL, "ic_comprehensive_stats_detrend_pieces, subint lines (%d entries): %s", nchan, e);
    PieceSpec ps{{0}, {0}};
    if (chan_npieces > 0) ps.cs.assign(chan_starts, chan_starts + chan_npieces);
    if (subint_npieces > 0) ps.ss.assign(subint_starts, subint_starts + subint_npieces);
    const TrendArgs dt{chan_order, subint_order, rounds, clip, chan_coef, subint_coef};
    return stats_oneshot(device, nsub, nchan, nbin, data, weights, chanthresh, subintthresh, test_out, std_o, mean_o,
                         nullptr, ptp_o, fftmax_o, 8, 1024, data_f64, &dt, &ps);
}

static int stats_oneshot(int device, int nsub, int nchan, int nbin, const float *data, const float *weights,
                         double chanthresh, double subintthresh, double *test_out, double *std_o, double *mean_o,
                         float *ptp_o, double *ptp64_o, double *fftmax_o, int rowstat_waves, int rowstat_minlen,
                         int data_f64, const TrendArgs *trend, const PieceSpec *pieces)
{
    if (!data || !weights || !test_out) return fail(IC_EINVAL, "null argument");
    if (rowstat_waves != 0 && rowstat_waves != 4 && rowstat_waves != 8)
        return fail(IC_EINVAL, "rowstat_waves=%d (0, 4 or 8)", rowstat_waves);
    if (rowstat_minlen < 1) return fail(IC_EINVAL, "rowstat_minlen=%d < 1", rowstat_minlen);
    if (nsub <= 0 || nchan <= 0 || nbin <= 0 || nsub > 16384 || nchan > 16384 || nbin > 32768)
        return fail(IC_EINVAL, "bad shape nsub=%d nchan=%d nbin=%d", nsub, nchan, nbin);
    if (diag_lds_bytes(nbin) > kLdsBlockMax) return fail(IC_EINVAL, "nbin=%d unsupported", nbin);
    if (int rc = select_device(device)) return rc;
    const size_t P = (size_t)nsub * nchan, N = P * (size_t)nbin;
    PwPlan plan;
    if (make_plan(nbin, &plan) != 0) return fail(IC_EINVAL, "pairwise plan too large for nbin=%d", nbin);
    const std::vector<double2> tw = host_twiddles(nbin), tw2 = p2_twiddles(nbin);
    const std::vector<double2> dt = diag_czt_supported(nbin) ? diag_czt_tables(nbin) : std::vector<double2>();
    Scratch sc;
    CK(sc.open_stream());
    hipStream_t st = sc.stream;
    float *D, *w0, *W, *hist;
    uint8_t *valid;
    double *sd, *mn, *ff, *pt, *test, *lstat, *coef;
    int32_t *cnt, *pstarts;
    int16_t *ppiece;
    const size_t mc = pieces ? pieces->cs.size() : 1, ms = pieces ? pieces->ss.size() : 1;
    const PieceTables ptab = pieces ? piece_tables(pieces->cs, pieces->ss, nsub, nchan) : PieceTables();
    double2 *dtw, *dtw2, *ddt;
    PwPlan *dplan;
    struct {
        void **p;
        size_t bytes;
    } al[] = {{(void **)&D, 4 * N},     {(void **)&w0, 4 * P},   {(void **)&valid, P},  {(void **)&W, 4 * P},
              {(void **)&hist, 8 * P},  {(void **)&sd, 8 * P},   {(void **)&mn, 8 * P}, {(void **)&ff, 8 * P},
              {(void **)&pt, 8 * P},    {(void **)&test, 8 * P}, {(void **)&lstat, 8 * 16 * ((size_t)nsub + nchan)},
              {(void **)&cnt, 4 * 8},   {(void **)&dtw, 16 * (size_t)nbin}, {(void **)&dtw2, 16 * (size_t)nbin + 16},
              {(void **)&dplan, sizeof plan}, {(void **)&ddt, 16 * dt.size()},
              {(void **)&coef, trend ? 8 * 16 * ((size_t)nsub * ms + (size_t)nchan * mc) : 0},
              {(void **)&pstarts, 4 * ptab.starts.size()}, {(void **)&ppiece, 2 * ptab.piece.size()}};
    for (auto &x : al)
        if (sc.mem.alloc_bytes(x.p, x.bytes + 16) != hipSuccess) return fail(IC_ENOMEM, "hipMalloc(%zu) failed", x.bytes);
    CK(hipMemcpyAsync(D, data, 4 * N, hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(w0, weights, 4 * P, hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(dtw, tw.data(), 16 * (size_t)nbin, hipMemcpyHostToDevice, st));
    if (!tw2.empty()) CK(hipMemcpyAsync(dtw2, tw2.data(), 16 * tw2.size(), hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(dplan, &plan, sizeof plan, hipMemcpyHostToDevice, st));
    if (!dt.empty()) CK(hipMemcpyAsync(ddt, dt.data(), 16 * dt.size(), hipMemcpyHostToDevice, st));
    CK(hipMemsetAsync(cnt, 0, 4 * 8, st));
    CK(launch_valid(st, w0, valid, W, hist, P));
    DiagArgs a{};
    a.mode = DIAG_STATS;
    a.D = D;
    a.ldD = nbin;
    a.w0 = w0;
    a.tw = dtw;
    a.tw_p2 = dtw2;
    a.plan = dplan;
    a.czt = dt.empty() ? nullptr : ddt;
    a.nsub = nsub;
    a.nchan = nchan;
    a.nbin = nbin;
    a.std_o = sd;
    a.mean_o = mn;
    a.fft_o = ff;
    a.ptp_o = pt;
    a.data_f64 = data_f64;
    CK(launch_diag(st, a));
    CombineArgs c;
    LineStatsArgs &la = c.ls;
    lay_lstat(&la, nsub, nchan, lstat);
    la.valid = valid;
    la.std_d = sd;
    la.mean_d = mn;
    la.fft_d = ff;
    la.ptp_d = pt;
    la.ptp_f32 = !data_f64;
    la.grp_waves = rowstat_waves;
    la.grp_minlen = rowstat_minlen;
    c.info = nullptr;
    c.w0 = w0;
    c.chanthresh = chanthresh;
    c.subintthresh = subintthresh;
    c.test = test;
    c.W = W;
    c.hist = hist;
    c.iter = 1;
    c.counters = cnt;
    c.grid_cap = 0;
    TrendArgs ta{};
    PieceArgs pa{};
    if (trend) {
        ta = *trend;
        ta.col_coef = coef;
        ta.row_coef = coef + (size_t)16 * nchan * mc;
        c.trend = &ta;
    }
    if (trend && pieces) {
        CK(hipMemcpyAsync(pstarts, ptab.starts.data(), 4 * ptab.starts.size(), hipMemcpyHostToDevice, st));
        CK(hipMemcpyAsync(ppiece, ptab.piece.data(), 2 * ptab.piece.size(), hipMemcpyHostToDevice, st));
        pa = piece_args(pieces->cs, pieces->ss, nsub, pstarts, ppiece);
        c.pieces = &pa;
    }
    CK(launch_lines(st, la, c.trend, c.pieces, 3));
    CK(launch_combine(st, c));
    if (trend && trend->col_coef)
        CK(hipMemcpyAsync(trend->col_coef, ta.col_coef, 8 * 16 * (size_t)nchan * mc, hipMemcpyDeviceToHost, st));
    if (trend && trend->row_coef)
        CK(hipMemcpyAsync(trend->row_coef, ta.row_coef, 8 * 16 * (size_t)nsub * ms, hipMemcpyDeviceToHost, st));
    CK(hipMemcpyAsync(test_out, test, 8 * P, hipMemcpyDeviceToHost, st));
    if (std_o) CK(hipMemcpyAsync(std_o, sd, 8 * P, hipMemcpyDeviceToHost, st));
    if (mean_o) CK(hipMemcpyAsync(mean_o, mn, 8 * P, hipMemcpyDeviceToHost, st));
    std::vector<double> ptp64(ptp_o ? P : 0);
    if (ptp_o) CK(hipMemcpyAsync(ptp64.data(), pt, 8 * P, hipMemcpyDeviceToHost, st));
    if (ptp64_o) CK(hipMemcpyAsync(ptp64_o, pt, 8 * P, hipMemcpyDeviceToHost, st));
    if (fftmax_o) CK(hipMemcpyAsync(fftmax_o, ff, 8 * P, hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    for (size_t k = 0; k < ptp64.size(); ++k) ptp_o[k] = (float)ptp64[k];
    return IC_OK;
}

// remove_profile1d (iterative_cleaner.py:275-288) over caller-given profiles:
// a one-shot session of nsub x nchan >= nprof profiles (zero rows pad the last
// subint) whose fit cube is the profiles themselves, then the session's fit
// (exact: run_fit; closed form: the fused kernel on raw rows with a zero
// baseline) and k_residual with no dispersion shift.
int ic_fit_profiles(int device, int nprof, int nbin, const float *T, const float *profiles, int fit_mode,
                    double *amp_out, int32_t *info_out, float *resid_out)
{
    if (!T || !profiles || (!amp_out && !info_out && !resid_out)) return fail(IC_EINVAL, "null argument");
    if (nprof <= 0 || nbin <= 0) return fail(IC_EINVAL, "bad shape nprof=%d nbin=%d", nprof, nbin);
    ic_params p{};
    p.nchan = nprof < 4096 ? nprof : 4096;
    p.nsub = (nprof + p.nchan - 1) / p.nchan;
    p.nbin = nbin;
    p.max_iter = 1;
    p.chanthresh = p.subintthresh = 5.0;
    p.baseline_duty = 0.15;
    p.fit_mode = fit_mode;
    void *h = nullptr;
    int rc = create_session(&p, device, 0, 1, false, [](std::string *, int *) -> Comm * { return nullptr; }, &h);
    if (rc) return rc;
    Session *s = (Session *)h;
    struct Guard {
        Session *s;
        ~Guard() { ic_session_destroy(s); }
    } guard{s};
    s->dtiled = 0;   // D is filled row by row below
    const size_t P = s->P, row = sizeof(float) * (size_t)nbin;
    std::vector<double> t64(s->ldD, 0.0);
    for (int i = 0; i < nbin; ++i) t64[i] = (double)T[i];
    CK(hipMemcpyAsync(s->T64, t64.data(), sizeof(double) * s->ldD, hipMemcpyHostToDevice, s->stream));
    CK(hipMemcpyAsync(s->T2, t64.data(), sizeof(double) * nbin, hipMemcpyHostToDevice, s->stream));
    CK(hipMemcpyAsync(s->T2 + nbin, t64.data(), sizeof(double) * nbin, hipMemcpyHostToDevice, s->stream));
    CK(hipMemsetAsync(s->shift, 0, sizeof(int32_t) * s->nchan, s->stream));
    CK(hipMemsetAsync(s->base0, 0, sizeof(float) * P, s->stream));
    {
        std::vector<float> ones(P, 1.0f);
        CK(hipMemcpyAsync(s->w0, ones.data(), sizeof(float) * P, hipMemcpyHostToDevice, s->stream));
        CK(hipStreamSynchronize(s->stream));
    }
    CK(hipMemsetAsync(s->raw, 0, sizeof(float) * s->N, s->stream));
    CK(hipMemcpyAsync(s->raw, profiles, row * nprof, hipMemcpyHostToDevice, s->stream));
    if (fit_mode == IC_FIT_EXACT) {
        CK(hipMemcpy2DAsync(s->D, sizeof(float) * s->ldD, s->raw, row, row, P, hipMemcpyDeviceToDevice, s->stream));
        if (int r = run_fit(s, nullptr)) return r;
    } else {
        CK(launch_tnorm(s->stream, s->T64, s->plan, s->plan_ub, s->TT));
        DiagArgs da = diag_args(s, 0, 0);
        CK(launch_diag(s->stream, da));
    }
    if (amp_out) CK(hipMemcpyAsync(amp_out, s->amp, sizeof(double) * nprof, hipMemcpyDeviceToHost, s->stream));
    if (info_out) CK(hipMemcpyAsync(info_out, s->info, sizeof(int32_t) * nprof, hipMemcpyDeviceToHost, s->stream));
    if (resid_out) {
        const auto bad = [](hipError_t e) { return named_fail("ic_fit_profiles residual", e); };
        Scratch tmp;
        float *R = nullptr;
        CK(tmp.mem.alloc_exact(&R, s->N));
        CKF(launch_residual(s->stream, s->D, s->raw, s->base0, s->T64, s->amp, s->info, s->shift, p.nsub, s->nchan,
                            nbin, s->ldD, s->dtiled, 0, 1.0, 0, 0, R, s->grid_cap), bad);
        CKF(hipMemcpyAsync(resid_out, R, row * nprof, hipMemcpyDeviceToHost, s->stream), bad);
        CKF(hipStreamSynchronize(s->stream), bad);   // before tmp frees R
    }
    CK(hipStreamSynchronize(s->stream));
    return IC_OK;
}

}  // extern "C"
