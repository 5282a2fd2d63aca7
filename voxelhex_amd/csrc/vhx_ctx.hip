// libvhx device side, context unit: context lifecycle, the tree-write ordering, scheduling settings and the tuning
// parser, streams and synchronisation, and the multi-GPU untile step.
//
// Kernels
//   k_untile_planes   scatters rank-gathered tile buffers into the framebuffers (multi-GPU screen-tile split)
// Launches no kernel of another unit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vhx.h"
#include "ctx.hpp"

using namespace vhx;

// Scatters rank-gathered tile buffers into framebuffers. Rank r's part of `gathered` holds `planes` planes of
// tiles_per_rank*T*T words each (plane 0 RGBA8, plane 1 f32 depth bits), rank r traced tiles r, r + ranks, ...
__global__ void __launch_bounds__(256) k_untile_planes(const uint32_t *__restrict__ gathered, uint32_t planes,
                                                       uint32_t ranks, uint32_t tiles_per_rank, uint32_t T,
                                                       uint32_t tiles_x, uint32_t ntiles, uint32_t width,
                                                       uint32_t height, uint32_t *__restrict__ fb0,
                                                       uint32_t *__restrict__ fb1) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t per_plane = (uint64_t)tiles_per_rank * T * T, per_rank = per_plane * planes;
    if (i >= per_rank * ranks) return;
    const uint32_t r = (uint32_t)(i / per_rank);
    const uint64_t w = i - (uint64_t)r * per_rank;
    const uint32_t plane = (uint32_t)(w / per_plane);
    const uint64_t k = w - (uint64_t)plane * per_plane;
    uint32_t *fb = plane ? fb1 : fb0;
    if (!fb) return;
    const uint32_t j = (uint32_t)(k / ((uint64_t)T * T));
    const uint32_t local = (uint32_t)(k - (uint64_t)j * T * T);
    const uint32_t tile = r + j * ranks;
    if (tile >= ntiles) return;
    const uint32_t px = (tile % tiles_x) * T + local % T, py = (tile / tiles_x) * T + local / T;
    if (px >= width || py >= height) return;
    fb[(uint64_t)py * width + px] = gathered[i];
}

TreeStore::~TreeStore() {
    (void)hipSetDevice(device);
    if (write_ev) (void)hipEventDestroy(write_ev);
    for (auto &b : raw)
        if (b.ptr) (void)hipFree(b.ptr);
    for (DevBuf *b : {&hdr, &brick_occ, &child_rec, &mips})
        if (b->ptr) (void)hipFree(b->ptr);
}

int vhx::ensure(vhx_ctx *c, DevBuf &b, uint64_t bytes) {
    if (b.bytes >= bytes && b.ptr) return VHX_OK;
    if (b.ptr) VHX_HIP(c, hipFree(b.ptr));
    b.ptr = nullptr;
    b.bytes = 0;
    if (bytes == 0) bytes = 16;
    VHX_HIP(c, hipMalloc(&b.ptr, bytes));
    b.bytes = bytes;
    return VHX_OK;
}

// ---- tree-write ordering (TreeStore): frames in flight on shared contexts and writes through the owner ----------
// VHX_UNORDERED_WRITES=1 (a diagnostic build only, never the shipped library: voxelhex_amd._build.build(defines=
// ("VHX_UNORDERED_WRITES=1",), lib=...)): no waits either way, the behaviour before round 3, to show that
// tests/test_gpu_ordering.py detects the missing ordering
#ifndef VHX_UNORDERED_WRITES
#define VHX_UNORDERED_WRITES 0
#endif
static constexpr bool unordered_writes() { return VHX_UNORDERED_WRITES != 0; }

// Writes and traces of one tree may come from several host threads (one per context): a write waits until no trace is
// between trace_begin and trace_end (a trace in submission is not yet visible in its use event), and a trace waits
// until no write is between write_begin and write_end, so every frame sees the tree as of its submission.
int vhx::write_begin(vhx_ctx *c) {
    TreeStore &ts = *c->tree;
    std::unique_lock<std::mutex> lock(ts.mu);
    // a waiting writer holds off traces that have not begun yet (trace_begin waits while writers_waiting > 0), so that
    // a stream of back-to-back traces from other threads cannot keep `tracing` above 0 forever
    ++ts.writers_waiting;
    ts.cv.wait(lock, [&] { return ts.tracing == 0 && ts.writing == 0; });
    --ts.writers_waiting;
    ++ts.writing;
    if (unordered_writes()) return VHX_OK;
    // every other context's last submitted trace, whatever stream it went to (waiting on an event of c's own stream is
    // a no-op, so no stream comparison: a context moved between streams by vhx_set_stream is still waited for)
    for (vhx_ctx *u : ts.users)
        if (u != c && u->use_recorded) VHX_HIP(c, hipStreamWaitEvent(c->stream, u->use_ev, 0));
    // a write on another stream than the previous write also follows it (writes are ordered among themselves)
    if (ts.write_seq && ts.write_stream != c->stream) VHX_HIP(c, hipStreamWaitEvent(c->stream, ts.write_ev, 0));
    return VHX_OK;
}

int vhx::write_end(vhx_ctx *c) {
    TreeStore &ts = *c->tree;
    std::lock_guard<std::mutex> lock(ts.mu);
    ts.writing = ts.writing > 0 ? ts.writing - 1 : 0;
    ts.cv.notify_all();
    // recorded on every exit (also after a failed write: the next traces wait for whatever it enqueued)
    if (!ts.write_ev) VHX_HIP(c, hipEventCreateWithFlags(&ts.write_ev, hipEventDisableTiming));
    VHX_HIP(c, hipEventRecord(ts.write_ev, c->stream));
    ts.write_stream = c->stream;
    ++ts.write_seq;
    c->seen_write = ts.write_seq;
    return VHX_OK;
}

int vhx::trace_begin(vhx_ctx *c) {
    TreeStore &ts = *c->tree;
    std::unique_lock<std::mutex> lock(ts.mu);
    ts.cv.wait(lock, [&] { return ts.writing == 0 && ts.writers_waiting == 0; });
    ++ts.tracing;
    if (unordered_writes()) return VHX_OK;
    if (c->seen_write != ts.write_seq) {
        if (ts.write_stream != c->stream) VHX_HIP(c, hipStreamWaitEvent(c->stream, ts.write_ev, 0));
        c->seen_write = ts.write_seq;
    }
    return VHX_OK;
}

int vhx::trace_end(vhx_ctx *c) {
    TreeStore &ts = *c->tree;
    std::lock_guard<std::mutex> lock(ts.mu);  // write_begin reads use_recorded / waits on use_ev
    ts.tracing = ts.tracing > 0 ? ts.tracing - 1 : 0;
    ts.cv.notify_all();
    if (!c->use_ev) VHX_HIP(c, hipEventCreateWithFlags(&c->use_ev, hipEventDisableTiming));
    VHX_HIP(c, hipEventRecord(c->use_ev, c->stream));
    c->use_stream = c->stream;
    c->use_recorded = true;
    return VHX_OK;
}

static void register_user(vhx_ctx *c) {
    std::lock_guard<std::mutex> lock(c->tree->mu);
    c->tree->users.push_back(c);
    c->seen_write = 0;  // the first trace waits for the tree's last write (if any, and on another stream)
}

static void unregister_user(vhx_ctx *c) {
    std::lock_guard<std::mutex> lock(c->tree->mu);
    auto &u = c->tree->users;
    u.erase(std::remove(u.begin(), u.end(), c), u.end());
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" {

uint32_t vhx_abi_version(void) { return VHX_ABI_VERSION; }

// The HIP runtime's answer, with its error: hipGetDeviceCount failing for any reason other than "no device" is
// VHX_E_HIP (count 0) and its text is kept for vhx_device_error (there is no context to hold it), instead of a silent
// count of 0 (a process that lost the device must say why)
static thread_local std::string g_device_err;
int vhx_device_count(int *count) {
    if (!count) return VHX_E_INVALID_ARG;
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e == hipErrorNoDevice) n = 0;  // no GPU visible: a count of 0, not an error (a CPU-only host)
    else if (e != hipSuccess) {
        g_device_err = std::string("hipGetDeviceCount: ") + hipGetErrorName(e) + ": " + hipGetErrorString(e);
        *count = 0;
        return VHX_E_HIP;
    }
    g_device_err.clear();
    *count = n;
    return VHX_OK;
}

const char *vhx_device_error(void) { return g_device_err.c_str(); }

int vhx_create(int hip_device, vhx_ctx **out) {
    if (!out) return VHX_E_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return VHX_E_NO_DEVICE;
    if (hip_device < 0 || hip_device >= n) return VHX_E_INVALID_ARG;
    vhx_ctx *c = new vhx_ctx();
    c->device = hip_device;
    c->tree = std::make_shared<TreeStore>();
    c->tree->device = hip_device;
    register_user(c);
    auto bail = [&](const char *what, hipError_t e) {
        fprintf(stderr, "vhx_create: %s: %s\n", what, hipGetErrorString(e));
        delete c;
        return VHX_E_HIP;
    };
    hipError_t e;
    if ((e = hipSetDevice(hip_device)) != hipSuccess) return bail("hipSetDevice", e);
    // no stream yet: the caller's (vhx_set_stream) or the context's own, created at first use (VHX_STREAM). The
    // library reads no environment: the schedule is the adaptive default until vhx_set_pass_budgets / vhx_set_tuning.
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, hip_device) == hipSuccess && prop.multiProcessorCount > 0) {
            c->cus = (uint32_t)prop.multiProcessorCount;
            c->queue_blocks = c->cus * 8u;
            c->queue_waves = c->sched_busy.queue_waves_per_cu * c->cus;
        }
    }
    if ((e = hipEventCreate(&c->ev0)) != hipSuccess) return bail("hipEventCreate", e);
    if ((e = hipEventCreate(&c->ev1)) != hipSuccess) return bail("hipEventCreate", e);
    *out = c;
    return VHX_OK;
}

int vhx_create_shared(const vhx_ctx *owner, vhx_ctx **out) {
    if (!owner || !out) return VHX_E_INVALID_ARG;
    *out = nullptr;
    vhx_ctx *c = nullptr;
    int rc = vhx_create(owner->device, &c);
    if (rc) return rc;
    c->tree = owner->tree;  // the same device tree (reference-counted); the context's fresh store goes with it
    register_user(c);
    c->shared = true;
    copy_sched(c, owner);  // the owner's scheduling settings (as of now; vhx_mgpu re-copies them per frame)
    *out = c;
    return VHX_OK;
}

void vhx_destroy(vhx_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    unregister_user(c);
    c->tree.reset();  // frees the device tree with its last context
    if (c->use_ev) (void)hipEventDestroy(c->use_ev);
    for (DevBuf *b : {&c->scratch, &c->rays, &c->queue[0], &c->queue[1], &c->qctl, &c->tmp, &c->counts, &c->offsets,
                      &c->flags, &c->qargs, &c->state, &c->stateq, &c->upd, &c->prepass_depth, &c->batch_args, &c->scan_part,
                      &c->shadow_args, &c->tail_list[0], &c->tail_list[1], &c->tail_mask, &c->build.occ, &c->build.rank,
                      &c->build.first, &c->build.part, &c->build.table, &c->build.ctl, &c->build.grid,
                      &c->build.simp, &c->build.dtable, &c->work, &c->query, &c->edit.oldn, &c->edit.aft, &c->edit.need,
                      &c->edit.rank, &c->edit.nmask, &c->edit.first, &c->edit.ctl, &c->points.in, &c->points.cur,
                      &c->points.idx, &c->points.mask, &c->points.first, &c->points.oldn, &c->points.aft,
                      &c->points.need, &c->points.rank, &c->points.ltype, &c->points.lu, &c->points.nmask,
                      &c->points.bfirst, &c->points.binfo, &c->points.bcnt, &c->points.bseg, &c->points.bflag,
                      &c->points.ctl, &c->compact.new_of,
                      &c->compact.old_of, &c->compact.nmask, &c->compact.nrank, &c->compact.bmask,
                      &c->compact.bfirst, &c->compact.bnew, &c->compact.bsrc, &c->compact.ctl, &c->simplify.binfo,
                      &c->simplify.pmask, &c->simplify.gmask, &c->simplify.bfirst, &c->simplify.ent,
                      &c->simplify.bsrc, &c->simplify.newb, &c->simplify.ctl, &c->palette.org, &c->palette.first,
                      &c->palette.map, &c->palette.ctl, &c->palette.dfirst, &c->palette.dmap, &c->list.fr[0],
                      &c->list.fr[1], &c->list.mask, &c->list.first, &c->list.unit, &c->list.ucnt, &c->list.part, &c->list.ctl, &c->list.out,
                      &c->lod.depth, &c->lod.pkey, &c->lod.mcol, &c->lod.has, &c->lod.binfo, &c->lod.bfirst,
                      &c->lod.bsrc, &c->lod.mips, &c->lod.ctl})
        if (b->ptr) (void)hipFree(b->ptr);
    if (c->tail_stream) {
        (void)hipStreamSynchronize(c->tail_stream);
        (void)hipStreamDestroy(c->tail_stream);
    }
    if (c->tail_fork) (void)hipEventDestroy(c->tail_fork);
    if (c->tail_join) (void)hipEventDestroy(c->tail_join);
    std::vector<vhx_ctx::Pinned *> pins = {&c->pinned[0], &c->pinned[1]};
    for (auto &P : c->batch_pinned) pins.push_back(&P);
    for (auto &P : c->shadow_pinned) pins.push_back(&P);
    for (auto *P : pins) {
        if (P->ptr) (void)hipHostFree(P->ptr);
        if (P->done) (void)hipEventDestroy(P->done);
    }
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

// vhx_set_tuning: the scheduling knobs of the probes (they used to be environment variables read at vhx_create; the
// library now reads none). Parsed into a copy of the context first, so a malformed spec changes nothing.
static bool parse_u32_list(const std::string &v, uint32_t *out, uint32_t cap, uint32_t &n) {
    n = 0;
    const char *q = v.c_str();
    if (!*q) return true;
    for (;;) {
        char *end = nullptr;
        const unsigned long x = strtoul(q, &end, 10);
        if (end == q || n >= cap || x > 0xFFFFFFFFul) return false;
        out[n++] = (uint32_t)x;
        if (*end == '\0') return true;
        if (*end != ',') return false;
        q = end + 1;
    }
}
static bool parse_u32(const std::string &v, uint32_t &out) {
    uint32_t n = 0, x[1];
    if (!parse_u32_list(v, x, 1, n) || n != 1) return false;
    out = x[0];
    return true;
}
static int apply_tuning(vhx_ctx *c, const std::string &key, const std::string &val) {
    uint32_t x = 0, n = 0, l[VHX_MAX_BUDGETS + 1];
    auto bad = [&]() { return fail(c, VHX_E_INVALID_ARG, ("vhx_set_tuning: bad value for " + key).c_str()); };
    if (key == "budgets") {  // "" or "0" = one pass
        if (!parse_u32_list(val, l, VHX_MAX_BUDGETS, n)) return bad();
        if (n == 1 && l[0] == 0) n = 0;
        return vhx_set_pass_budgets(c, l, n);
    } else if (key == "adaptive") {
        if (!parse_u32(val, x) || x > 1) return bad();
        return vhx_set_adaptive_schedule(c, (int)x);
    } else if (key == "rpw") {  // queue passes 1.., 0 = adaptive
        if (!parse_u32_list(val, l, VHX_MAX_BUDGETS, n)) return bad();
        for (uint32_t i = 0; i < n; ++i) {
            if (l[i] > 64) return bad();
            c->rpw[i + 1] = l[i];
        }
    } else if (key == "tw") {
        if (!parse_u32(val, x) || x == 0) return bad();
        c->tw = x;
    } else if (key == "xcdg") {
        if (!parse_u32(val, x)) return bad();
        c->xcd_group = x;
    } else if (key == "resume") {
        if (!parse_u32(val, x) || x > 1) return bad();
        c->resume = x != 0;
    } else if (key == "tlists") {
        if (!parse_u32(val, x) || x > 1) return bad();
        c->tile_lists = x != 0;
    } else if (key == "qstate") {
        if (!parse_u32(val, x) || x > 1) return bad();
        c->qstate = x != 0;
    } else if (key == "save_from") {
        if (!parse_u32(val, x)) return bad();
        c->save_from = x;
    } else if (key == "qblock") {
        if (!parse_u32(val, x) || (x != 64 && x != 128 && x != 256)) return bad();
        c->qblock = x;
    } else if (key == "qwaves") {  // fixes the schedule
        if (!parse_u32(val, x) || x == 0) return bad();
        if (c->adaptive) vhx_set_adaptive_schedule(c, 0);
        c->queue_waves = x;
    } else if (key == "qwpc_idle" || key == "qwpc_busy") {  // queue waves per CU of one schedule (stays adaptive)
        if (!parse_u32(val, x) || x == 0 || x > 64) return bad();
        (key == "qwpc_idle" ? c->sched_idle : c->sched_busy).queue_waves_per_cu = x;
    } else if (key == "qwavesm") {
        if (!parse_u32(val, x)) return bad();
        c->queue_waves_mid = x;
    } else if (key == "p0lists") {  // pass 0 of primary frames: 1 = lists in the queue order (ListOrder), 0 = flags
        if (!parse_u32(val, x) || x > 1) return bad();
        c->p0lists = x != 0;
    } else if (key == "scan_multi") {  // 0 = every scan on one workgroup
        if (!parse_u32(val, x)) return bad();
        c->scan_multi = x;
    } else if (key == "tail") {  // early tail of lone frames (vhx_ctx::tail_*): 1 on, 0 off
        if (!parse_u32(val, x) || x > 1) return bad();
        c->tail_on = x != 0;
    } else if (key == "tail_min") {  // steps from which a ray joins the next lone frame's early tail
        if (!parse_u32(val, x) || x == 0) return bad();
        c->tail_min = x;
    } else if (key == "tail_rpw") {  // early-tail rays per wave
        if (!parse_u32(val, x) || x == 0 || x > 64) return bad();
        c->tail_rpw = x;
    } else if (key == "tail_prio") {  // s_setprio of the early-tail waves (0-3)
        if (!parse_u32(val, x) || x > 3) return bad();
        c->tail_prio = x;
    } else if (key == "tail_cap") {  // longest list recorded
        if (!parse_u32(val, x) || x > (1u << 20)) return bad();
        c->tail_cap = x;
        c->tail_valid = false;  // (a list recorded under another cap may hold more entries)
    } else if (key == "finter") {  // batches: pass-0 blocks of the frames interleaved (1) or frame-major (0)
        if (!parse_u32(val, x) || x > 1) return bad();
        c->frame_interleave = x != 0;
    } else if (key == "skyblocks") {  // batches: pass 0 over a worklist, tree blocks first, all-sky blocks last (1) or every block alike (0)
        if (!parse_u32(val, x) || x > 1) return bad();
        c->skyblocks = x != 0;
    } else if (key == "stage_slots") {  // batch staging ring slots in use (1 = wait for the previous batch's copy)
        if (!parse_u32(val, x) || x == 0 || x > vhx_ctx::VHX_STAGE_SLOTS) return bad();
        c->stage_slots = x;
    } else if (key == "sbudget") {  // fused shadows: steps of a shadow ray in its primary ray's pass (0 = the rest)
        if (!parse_u32(val, x)) return bad();
        c->shadow_budget = x;
    } else if (key == "qwaves0") {
        if (!parse_u32(val, x) || x == 0) return bad();
        c->queue_waves0 = c->queue_waves0_force = x;
    } else if (key == "qxcd") {
        if (!parse_u32(val, x)) return bad();
        c->qxcd = x;
    } else if (key == "qxcd_all") {
        if (!parse_u32(val, x) || x > 1) return bad();
        c->qxcd_all = x != 0;
    } else if (key == "sparse") {  // per budgeted pass; fixes the schedule
        if (!parse_u32_list(val, l, VHX_MAX_BUDGETS, n)) return bad();
        for (uint32_t i = 0; i < n; ++i)
            if (l[i] > 64) return bad();
        if (c->adaptive) vhx_set_adaptive_schedule(c, 0);
        for (uint32_t i = 0; i < VHX_MAX_BUDGETS; ++i) c->sparse[i] = i < n ? l[i] : 0u;
    } else if (key == "qorder") {  // "[m]N[z|r]": NxN tiles, (m) Morton order of the tiles, (z) Morton / (r) rows inside
        const bool m = !val.empty() && val[0] == 'm';
        char *end = nullptr;
        const char *b = val.c_str() + (m ? 1 : 0);
        const long ts = strtol(b, &end, 10);
        if (end == b) return bad();
        const bool z = *end == 'z', rows = *end == 'r';
        if (*end && !((z || rows) && end[1] == '\0')) return bad();
        uint32_t lg = 0;
        while (lg < 12u && (1l << lg) < ts) ++lg;
        uint32_t code = 0;
        if (ts != 0) {
            if (ts < 8 || ts > 4096 || (1l << lg) != ts) return bad();
            code = lg | (m ? 16u : 0u) | (z ? 32u : 0u) | (rows ? 64u : 0u);
        }
        c->qorder = c->sched_busy.qorder = c->sched_idle.qorder = code;  // both schedules (the rest stays adaptive)
    } else if (key == "qsort") {  // segment length of the queue passes' node sort: 0 = off, else 256 .. VHX_QSORT_MAX
        if (!parse_u32(val, x) || (x && (x < 256 || x > VHX_QSORT_MAX || (x & (x - 1))))) return bad();
        c->qsort_force = (int)x;
    } else if (key == "qsortp") {  // bit mask of the queue passes whose input is sorted
        if (!parse_u32(val, x)) return bad();
        c->qsort_passes = x;
    } else if (key == "qsortb") {
        if (!parse_u32(val, x) || x == 0) return bad();
        c->qsort_blocks = x;
    } else {
        return fail(c, VHX_E_INVALID_ARG, ("vhx_set_tuning: unknown key " + key).c_str());
    }
    return VHX_OK;
}

int vhx_set_tuning(vhx_ctx *c, const char *spec) {
    if (!c || !spec) return VHX_E_INVALID_ARG;
    std::vector<std::pair<std::string, std::string>> kv;
    for (const char *q = spec; *q;) {
        const char *e = q;
        while (*e && *e != ';') ++e;
        const std::string item(q, e);
        q = *e ? e + 1 : e;
        if (item.empty()) continue;
        const size_t eq = item.find('=');
        if (eq == std::string::npos || eq == 0) return fail(c, VHX_E_INVALID_ARG, "vhx_set_tuning: expected key=value");
        kv.emplace_back(item.substr(0, eq), item.substr(eq + 1));
    }
    // a dry run on a scratch context first: a malformed spec leaves c unchanged
    {
        vhx_ctx dry;
        copy_sched(&dry, c);
        for (const auto &p : kv) {
            const int rc = apply_tuning(&dry, p.first, p.second);
            if (rc) {
                c->err = dry.err;
                return rc;
            }
        }
    }
    for (const auto &p : kv) {
        const int rc = apply_tuning(c, p.first, p.second);
        if (rc) return rc;
    }
    return VHX_OK;
}

int vhx_set_adaptive_schedule(vhx_ctx *c, int on) {
    if (!c) return VHX_E_INVALID_ARG;
    if (!on && c->adaptive) {  // leaving the adaptive choice: the frames-in-flight schedule, whatever the last trace ran
        const vhx_ctx::Sched &s = c->sched_busy;
        std::memcpy(c->budgets, s.budgets, sizeof(c->budgets));
        std::memcpy(c->sparse, s.sparse, sizeof(c->sparse));
        c->npass = s.npass;
        c->queue_waves = s.queue_waves_per_cu * c->cus;
        c->queue_waves0 = c->queue_waves0_force ? c->queue_waves0_force : s.queue_waves0_per_cu * c->cus;
        c->qorder = s.qorder;
        c->last_sched = -1;
    }
    c->adaptive = on != 0;
    return VHX_OK;
}

int vhx_get_pass_budgets(const vhx_ctx *c, uint32_t *budgets, uint32_t *n, int *sched) {
    if (!c || !n) return VHX_E_INVALID_ARG;
    *n = c->npass > 0 ? c->npass - 1 : 0;
    if (budgets)
        for (uint32_t i = 0; i < VHX_MAX_BUDGETS; ++i) budgets[i] = i < *n ? c->budgets[i] : 0u;
    if (sched) *sched = c->last_sched;
    return VHX_OK;
}

const char *vhx_last_error(const vhx_ctx *c) { return c ? c->err.c_str() : "null context"; }

int vhx_set_stream(vhx_ctx *c, void *s) {
    if (!c) return VHX_E_INVALID_ARG;
    c->stream = s ? (hipStream_t)s : c->own_stream;  // null own stream: created at the next use
    c->qargs_host_ptr[0] = c->qargs_host_ptr[1] = nullptr;  // written on the previous stream: rewrite them
    return VHX_OK;
}

int vhx_get_stream(vhx_ctx *c, void **s) {
    if (!c || !s) return VHX_E_INVALID_ARG;
    VHX_HIP(c, hipSetDevice(c->device));
    VHX_STREAM(c);
    *s = (void *)c->stream;
    return VHX_OK;
}

int vhx_sync(vhx_ctx *c, float *ms) {
    if (!c) return VHX_E_INVALID_ARG;
    VHX_HIP(c, hipSetDevice(c->device));
    if (c->stream) VHX_HIP(c, hipStreamSynchronize(c->stream));
    if (ms) {
        *ms = 0.f;
        if (c->timed) VHX_HIP(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    }
    return VHX_OK;
}

}  // extern "C"

int vhx::launch_untile(vhx_ctx *c, hipStream_t stream, const void *gathered, uint32_t planes, uint32_t ranks,
                       uint32_t tiles_per_rank, uint32_t T, uint32_t width, uint32_t height, uint32_t *fb_rgba,
                       float *fb_depth) {
    const uint32_t tiles_x = (width + T - 1) / T, tiles_y = (height + T - 1) / T;
    const uint64_t n = (uint64_t)ranks * planes * tiles_per_rank * T * T;
    if (n == 0) return VHX_OK;
    k_untile_planes<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>((const uint32_t *)gathered, planes, ranks,
                                                                     tiles_per_rank, T, tiles_x, tiles_x * tiles_y,
                                                                     width, height, fb_rgba, (uint32_t *)fb_depth);
    VHX_HIP(c, hipGetLastError());
    return VHX_OK;
}

void vhx::copy_sched(vhx_ctx *c, const vhx_ctx *owner) {
    std::memcpy(c->budgets, owner->budgets, sizeof(c->budgets));
    std::memcpy(c->rpw, owner->rpw, sizeof(c->rpw));
    c->npass = owner->npass;
    c->tw = owner->tw;
    c->scan_multi = owner->scan_multi;
    c->p0lists = owner->p0lists;
    c->resume = owner->resume;
    c->qstate = owner->qstate;
    c->tile_lists = owner->tile_lists;
    c->save_from = owner->save_from;
    c->qorder = owner->qorder;
    c->adaptive = owner->adaptive;
    c->sched_busy = owner->sched_busy;
    c->sched_idle = owner->sched_idle;
    c->cus = owner->cus;
    c->xcd_group = owner->xcd_group;
    c->qblock = owner->qblock;
    c->queue_blocks = owner->queue_blocks;
    c->queue_waves = owner->queue_waves;
    c->queue_waves0 = owner->queue_waves0;
    c->queue_waves0_force = owner->queue_waves0_force;
    c->shadow_budget = owner->shadow_budget;
    c->stage_slots = owner->stage_slots;
    c->frame_interleave = owner->frame_interleave;
    c->skyblocks = owner->skyblocks;
    c->tail_on = owner->tail_on;
    c->tail_min = owner->tail_min;
    c->tail_rpw = owner->tail_rpw;
    c->tail_prio = owner->tail_prio;
    if (c->tail_cap != owner->tail_cap) c->tail_valid = false;
    c->tail_cap = owner->tail_cap;
    c->queue_waves_mid = owner->queue_waves_mid;
    c->qxcd = owner->qxcd;
    c->qxcd_all = owner->qxcd_all;
    c->qsort_force = owner->qsort_force;
    c->qsort_passes = owner->qsort_passes;
    c->qsort_blocks = owner->qsort_blocks;
    std::memcpy(c->sparse, owner->sparse, sizeof(c->sparse));
    c->prepass = owner->prepass;
    c->prepass_margin = owner->prepass_margin;
    c->shadow_on = owner->shadow_on;
    std::memcpy(c->shadow_light, owner->shadow_light, sizeof(c->shadow_light));
}

extern "C" {

int vhx_set_shadow_light(vhx_ctx *c, const float *light) {
    if (!c) return VHX_E_INVALID_ARG;
    if (light && !(std::isfinite(light[0]) && std::isfinite(light[1]) && std::isfinite(light[2])))
        return fail(c, VHX_E_INVALID_ARG, "vhx_set_shadow_light: a finite light position");
    c->shadow_on = light != nullptr;
    for (int k = 0; k < 3; ++k) c->shadow_light[k] = light ? light[k] : 0.0f;
    return VHX_OK;
}

int vhx_set_depth_prepass(vhx_ctx *c, int enable, float margin) {
    if (!c || !(margin >= 0.0f)) return VHX_E_INVALID_ARG;
    c->prepass = enable != 0;
    c->prepass_margin = margin;
    return VHX_OK;
}

int vhx_untile_frame(vhx_ctx *c, const void *gathered, uint32_t planes, uint32_t ranks, uint32_t tiles_per_rank,
                     uint32_t T, uint32_t width, uint32_t height, uint32_t *fb_rgba, float *fb_depth) {
    if (!c || !gathered || (!fb_rgba && !fb_depth) || planes < 1 || planes > 2 || (planes == 1 && fb_depth) ||
        ranks == 0 || T == 0 || width == 0 || height == 0)
        return fail(c, VHX_E_INVALID_ARG, "vhx_untile_frame: bad arguments");
    const uint32_t tiles_x = (width + T - 1) / T, tiles_y = (height + T - 1) / T;
    const uint64_t ntiles = (uint64_t)tiles_x * tiles_y;
    if (ntiles > 0xFFFFFFFFull || (uint64_t)tiles_per_rank * ranks < ntiles)
        return fail(c, VHX_E_INVALID_ARG, "vhx_untile_frame: tiles_per_rank * ranks does not cover the frame");
    const uint64_t n = (uint64_t)ranks * planes * tiles_per_rank * T * T;
    if ((n + 255) / 256 > 0x7FFFFFFFull) return fail(c, VHX_E_INVALID_ARG, "too many pixels");
    VHX_HIP(c, hipSetDevice(c->device));
    VHX_STREAM(c);
    return launch_untile(c, c->stream, gathered, planes, ranks, tiles_per_rank, T, width, height, fb_rgba, fb_depth);
}

int vhx_untile_rgba(vhx_ctx *c, const uint32_t *gathered, uint32_t ranks, uint32_t tiles_per_rank, uint32_t T,
                    uint32_t width, uint32_t height, uint32_t *fb, int on_device) {
    if (!c || !gathered || !fb || ranks == 0 || T == 0 || width == 0 || height == 0) return VHX_E_INVALID_ARG;
    if (!on_device) return fail(c, VHX_E_INVALID_ARG, "vhx_untile_rgba works on device buffers");
    return vhx_untile_frame(c, gathered, 1, ranks, tiles_per_rank, T, width, height, fb, nullptr);
}

}  // extern "C"
