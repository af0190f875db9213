// kifs_multi.cpp -- one process driving several devices (the reference's host is one process and one
// thread, application.rs:37-48): a kifs_multi owns one context per listed device.
//
//   kifs_multi_render              one frame: stripe shards, dense, synchronous (the latency form)
//   kifs_multi_render_batch_async  a step of up to 512 frames: ONE launch per device, the other devices' rows
//                                  packed into sparse records (or sent whole), gathered on the root by RCCL
//                                  grouped send/recv (or peer copies), two steps in flight
//
// How a step flows (S = 2 slots; device 0 is the root; every device has its context's render stream and a
// comm stream, the root also a gather stream):
//
//   submit(k)   host: complete step k - 2 (the slot's previous step: its payload buffers are free again)
//               root gather stream : background under the other devices' rows of the step's frames (fill, or
//                                    erase under the slot's previous records)
//               every render stream: render shard  [pack + record count to pinned memory] -> event packed[i]
//                                    (the root: in place into the frames -> event rendered)
//               then flush(k - 1)
//   flush(j)    host: wait packed[i] of step j, read the record counts (pinned memory)       -- by now every device
//               RCCL: GroupStart; device i comm stream: Send(records, root) ...; root gather   is rendering step j + 1
//                     stream: Recv(i) ...; GroupEnd          (COPY: hipMemcpyPeerAsync on the gather stream)
//               root gather stream : scatter the records (or unpack the stripes) -> event gathered
//   wait(j)     flush(j) if still pending; host waits for rendered and gathered of step j
//
// Nothing on a GPU waits for the host, and the host blocks only in flush (on work enqueued a step earlier).
// In the code, submit is check_step, complete_slot(k - 2), erase_suffices, paint_background, submit_device per device
// (abandon_step if one fails), advance_pipeline; flush is flush_slot; wait is flush_older, then complete_slot.
// Host code only; kernels live in kifs_kernels.hip / kifs_support_kernels.hip.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <new>
#include <set>
#include <vector>

#include <dlfcn.h>

#include "kifs_comm.hpp"
#include "kifs_context.hpp"

using namespace kifs::host;

// ---- RCCL, opened on first use -------------------------------------------------------------------------
namespace kifs {
namespace host {

const RcclApi* rccl() {
    static const RcclApi* api = []() -> const RcclApi* {
        const bool verbose = std::getenv("KIFS_DEBUG") != nullptr;
        void* h = nullptr;
        for (const char* name : {"librccl.so.1", "librccl.so"}) {
            h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (h) break;
        }
        if (!h) {
            if (verbose) std::fprintf(stderr, "kifs: dlopen(librccl.so.1) failed: %s\n", dlerror());
            return nullptr;
        }
        static RcclApi a;
        bool ok = true;
        auto sym = [&](auto& fn, const char* name) {
            fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(h, name));
            if (!fn) {
                ok = false;
                if (verbose) std::fprintf(stderr, "kifs: librccl lacks %s\n", name);
            }
        };
        sym(a.GetVersion, "ncclGetVersion");
        sym(a.CommInitAll, "ncclCommInitAll");
        sym(a.CommDestroy, "ncclCommDestroy");
        sym(a.GroupStart, "ncclGroupStart");
        sym(a.GroupEnd, "ncclGroupEnd");
        sym(a.Send, "ncclSend");
        sym(a.Recv, "ncclRecv");
        sym(a.GetErrorString, "ncclGetErrorString");
        if (!ok) return nullptr;
        int v = 0;
        if (a.GetVersion(&v) == ncclSuccess) a.version = v;
        return &a;
    }();
    return api;
}

bool nccl_ok(ncclResult_t r, const char* what) {
    if (r == ncclSuccess) return true;
    static const bool verbose = std::getenv("KIFS_DEBUG") != nullptr;
    if (verbose) {
        const RcclApi* a = rccl();
        std::fprintf(stderr, "kifs: %s failed: %s\n", what, a ? a->GetErrorString(r) : "?");
    }
    return false;
}

}  // namespace host
}  // namespace kifs

// ---- the object ------------------------------------------------------------------------------------------
namespace {

constexpr int SLOTS = 2;  // steps in flight

// A payload where it is packed and where it lands: both kifs_multi_render (one shard) and a step (`count` shards, or
// the sparse records' receive side) own one per non-root device.
struct Payload {
    uint8_t* shard = nullptr;  // on the device: packed shards, rows x W x 4 each
    uint8_t* recv = nullptr;   // on the root: the payload as received
    size_t shard_bytes = 0, recv_bytes = 0;
};

// Everything one listed device has for as long as the object lives ([0] is the root).
struct Device {
    int id = -1;
    kifs_ctx* ctx = nullptr;
    int weight = 1;                        // its share (kifs_shard_stripes weights)
    std::vector<int> stripes;              // its shard for the current frame height
    int rows = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // kernel start/stop on its render stream (latest launch)
    double shard_ms = -1.0;
    hipStream_t comm_stream = nullptr;     // batched steps; the root's is the gather stream
    ncclComm_t comm = nullptr;             // RCCL transport only
    Payload lone;                          // kifs_multi_render (non-root)
};

// What one device contributes to one step (device 0, the root, uses only `stripes` and `rows`).
struct PeerPart {
    std::vector<int> stripes;      // the device's shard when the step was submitted
    int rows = 0;
    Payload buf;                   // `count` packed shards; received: the shards (dense) or the records (sparse)
    uint8_t* records = nullptr;    // on the device: the sparse payload
    uint32_t* d_count = nullptr;   // on the device: number of records
    uint32_t* h_count = nullptr;   // pinned host copy
    hipEvent_t packed = nullptr;   // device's render stream: payload (and count) ready
    uint32_t n_records = 0;        // as flushed (sparse)
    size_t payload_bytes = 0;      // as flushed
    size_t records_bytes = 0;      // allocated
};

// What a step renders, and where to.
struct StepShape {
    int count = 0, encode = 0, gather = 0, width = 0, height = 0;
    uint8_t* frames = nullptr;
    size_t pitch = 0, stride = 0;
    uint32_t background = 0;
};

struct StepSlot : StepShape {
    bool used = false;             // holds a step that has not been completed by a wait
    bool flushed = false;
    uint64_t step = 0;
    bool background_known = false; // `frames` hold the background outside the records of `part` (sparse, flushed)
    bool overwritten = false;      // something else wrote into `frames` since this step was submitted
    std::vector<PeerPart> part;
    std::vector<int> peer_stripes; // every stripe that is not the root's, ascending
    hipEvent_t rendered = nullptr; // root render stream: the root's own rows are in the frames
    hipEvent_t gathered = nullptr; // root gather stream: everybody else's are
};

// One entry of a group of transfers to the root: `bytes` (0: nothing) from `src`, readable after `ready` (null: at once).
struct Transfer { const uint8_t* src; uint8_t* dst; size_t bytes; hipEvent_t ready; };

}  // namespace

struct kifs_multi {
    // never empty once created; the arrays ncclCommInitAll and kifs_shard_stripes want are built where they are called
    std::vector<Device> dev;
    int stripes_height = -1;
    uint8_t* root_frame = nullptr;         // staging frame on the root when the destination is host memory
    size_t root_frame_bytes = 0;
    // ---- batched steps
    int gather = KIFS_GATHER_SPARSE;
    int transport_wanted = KIFS_TRANSPORT_AUTO;
    int transport = KIFS_TRANSPORT_AUTO;   // decided at the first step (or by kifs_multi_set_gather)
    StepSlot slot[SLOTS];
    uint64_t next_step = 0;
    bool streams_tried = false;            // ensure_streams has run (its outcome stands, as it always has)
    bool have_pending = false;             // a submitted step whose transfers are not posted yet
    uint64_t pending = 0;
    std::vector<uint8_t*> outs_scratch;    // destination pointers of one device's launch
    KifsMultiStats stats{};
};

namespace {

// The two sides of a payload, before they are needed, and both gone.  `shard` is grown and the payload freed under the
// packing device; `recv` lives on the root.
bool grow_shard(Payload& b, size_t need, const char* what) { return grow(b.shard, b.shard_bytes, need, what); }
bool grow_recv(Payload& b, int root_id, size_t need, const char* what) {
    if (need <= b.recv_bytes) return true;
    DeviceGuard g(root_id);
    return grow(b.recv, b.recv_bytes, need, what);
}

void free_payload(Payload& b, int root_id) {
    if (b.shard) (void)hipFree(b.shard);
    if (b.recv) {
        DeviceGuard g(root_id);
        (void)hipFree(b.recv);
    }
    b = Payload();
}

// (Re)deal the frame's stripes to the devices.
int multi_partition(kifs_multi* m, int h) {
    if (m->stripes_height == h) return KIFS_OK;
    const int n = int(m->dev.size());
    const int all = (h + KIFS_STRIPE_ROWS - 1) / KIFS_STRIPE_ROWS;
    std::vector<int> weights;
    for (const Device& d : m->dev) weights.push_back(d.weight);
    for (int i = 0; i < n; ++i) {
        Device& d = m->dev[size_t(i)];
        d.stripes.assign(size_t(all), 0);
        int count = 0;
        int st = kifs_shard_stripes(h, n, weights.data(), i, d.stripes.data(), all, &count, &d.rows);
        if (st != KIFS_OK) return st;
        d.stripes.resize(size_t(count));
    }
    m->stripes_height = h;
    return KIFS_OK;
}

void destroy_comms(kifs_multi* m) {
    for (Device& d : m->dev) {
        if (!d.comm) continue;
        if (const RcclApi* a = rccl()) (void)a->CommDestroy(d.comm);
        d.comm = nullptr;
    }
    m->stats.comm_ranks = 0;
}

// Transport of the batched steps: decided once, communicators created on demand.
int ensure_transport(kifs_multi* m) {
    if (m->transport != KIFS_TRANSPORT_AUTO) return KIFS_OK;
    const int n = int(m->dev.size());
    std::vector<int> ids;
    for (const Device& d : m->dev) ids.push_back(d.id);
    const bool distinct = std::set<int>(ids.begin(), ids.end()).size() == ids.size();
    int want = m->transport_wanted;
    const bool automatic = want == KIFS_TRANSPORT_AUTO;
    if (automatic) want = (n >= 2 && distinct) ? KIFS_TRANSPORT_RCCL : KIFS_TRANSPORT_COPY;
    if (want == KIFS_TRANSPORT_RCCL) {
        // An explicit KIFS_TRANSPORT_RCCL that cannot be had is an error; AUTO falls back to peer copies (a node
        // without a loadable librccl, or whose ncclCommInitAll fails, still gathers) and says so under KIFS_DEBUG
        // and in stats.transport.
        auto give_up = [&](const char* why) {
            if (!automatic) return int(KIFS_ERR_COMM);
            if (std::getenv("KIFS_DEBUG")) std::fprintf(stderr, "kifs: %s; KIFS_TRANSPORT_AUTO falls back to peer copies\n", why);
            want = KIFS_TRANSPORT_COPY;
            return int(KIFS_OK);
        };
        int st = KIFS_OK;
        const RcclApi* a = nullptr;
        if (!distinct) st = give_up("a device is listed twice (ncclCommInitAll refuses that)");
        else if (!(a = rccl())) st = give_up("librccl could not be opened");
        else {
            std::vector<ncclComm_t> comms(size_t(n), nullptr);
            if (!nccl_ok(a->CommInitAll(comms.data(), n, ids.data()), "ncclCommInitAll")) {
                (void)hipGetLastError();
                st = give_up("ncclCommInitAll failed");
            } else {
                for (int i = 0; i < n; ++i) m->dev[size_t(i)].comm = comms[size_t(i)];
                m->stats.rccl_version = a->version;
                m->stats.comm_ranks = n;
            }
        }
        if (st != KIFS_OK) return st;
    }
    m->transport = m->stats.transport = want;
    return KIFS_OK;
}

int ensure_streams(kifs_multi* m) {
    if (m->streams_tried) return KIFS_OK;
    m->streams_tried = true;
    for (Device& d : m->dev) {
        DeviceGuard g(d.id);
        if (!g.ok || !hip_ok(hipStreamCreateWithFlags(&d.comm_stream, hipStreamNonBlocking), "comm stream"))
            return KIFS_ERR_RUNTIME;
    }
    return KIFS_OK;
}

inline int runtime_status(bool ok) { return ok ? KIFS_OK : KIFS_ERR_RUNTIME; }

bool make_event(hipEvent_t& ev) {
    return ev || hip_ok(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate(multi)");
}

// One group of point-to-point transfers: device i's x[i].src (x[i].bytes > 0) -> the root's x[i].dst, once x[i].ready
// has happened.  The receives (or the copies) are enqueued on the root's gather stream, so whatever follows there
// sees the data -- and once that has completed, every src has been read.
int transfer_to_root(kifs_multi* m, const std::vector<Transfer>& x, bool include_root) {
    const size_t n = m->dev.size();
    const Device& root = m->dev[0];
    hipStream_t gstream = root.comm_stream;
    const size_t first = include_root ? 0 : 1;
    if (m->transport == KIFS_TRANSPORT_RCCL) {
        const RcclApi* a = rccl();
        if (!a || !root.comm) return KIFS_ERR_COMM;
        for (size_t i = first; i < n; ++i) {
            if (!x[i].bytes || !x[i].ready) continue;
            DeviceGuard g(m->dev[i].id);
            if (!hip_ok(hipStreamWaitEvent(m->dev[i].comm_stream, x[i].ready, 0), "wait(payload ready)")) return KIFS_ERR_RUNTIME;
        }
        if (!nccl_ok(a->GroupStart(), "ncclGroupStart")) return KIFS_ERR_COMM;
        bool ok = true;
        for (size_t i = first; i < n && ok; ++i) {
            if (!x[i].bytes) continue;
            ok = nccl_ok(a->Send(x[i].src, x[i].bytes, ncclUint8, 0, m->dev[i].comm, m->dev[i].comm_stream), "ncclSend");
        }
        for (size_t i = first; i < n && ok; ++i) {
            if (!x[i].bytes) continue;
            ok = nccl_ok(a->Recv(x[i].dst, x[i].bytes, ncclUint8, int(i), root.comm, gstream), "ncclRecv");
        }
        const bool ended = nccl_ok(a->GroupEnd(), "ncclGroupEnd");
        return ok && ended ? KIFS_OK : KIFS_ERR_COMM;
    }
    // COPY: the root pulls every payload with the copy engines, one peer copy each, on its gather stream
    DeviceGuard g(root.id);
    for (size_t i = first; i < n; ++i) {
        if (!x[i].bytes) continue;
        if (x[i].ready && !hip_ok(hipStreamWaitEvent(gstream, x[i].ready, 0), "wait(payload ready)")) return KIFS_ERR_RUNTIME;
        const hipError_t e = m->dev[i].id == root.id
                                 ? hipMemcpyAsync(x[i].dst, x[i].src, x[i].bytes, hipMemcpyDeviceToDevice, gstream)
                                 : hipMemcpyPeerAsync(x[i].dst, root.id, x[i].src, m->dev[i].id, x[i].bytes, gstream);
        if (!hip_ok(e, "peer copy of a payload")) return KIFS_ERR_COMM;
    }
    return KIFS_OK;
}

// The dense scatter, on the root: the packed shards at `src` (one per frame of `s`, `shard_stride` apart) go to their
// stripes' rows of the frames.
int unpack_dense(const Device& root, hipStream_t stream, const StepShape& s, const uint8_t* src, size_t shard_stride,
                 const std::vector<int>& stripes) {
    const RowTable* rows = row_table(root.ctx, stripes.data(), int(stripes.size()), s.height);
    if (!rows) return KIFS_ERR_RUNTIME;
    return runtime_status(hip_ok(kifs::launch_unpack_stripes(s.frames, s.pitch, s.stride, src, size_t(s.width) * 4, shard_stride, rows->d_rows,
                                                             int(stripes.size()), s.count, s.width, s.height, stream),
                                 "unpack_stripes_kernel launch"));
}

// The sparse scatter, on the root's gather stream: the records received from `p` go to their tiles of the frames of
// `s` -- or, to erase them, the background does.
int unpack_records(const Device& root, const StepShape& s, const PeerPart& p, int erase, const char* what) {
    const RowTable* rows = row_table(root.ctx, p.stripes.data(), int(p.stripes.size()), s.height);
    if (!rows) return KIFS_ERR_RUNTIME;
    return runtime_status(hip_ok(kifs::launch_unpack_sparse(s.frames, s.pitch, s.stride, reinterpret_cast<const uint32_t*>(p.buf.recv),
                                                            p.n_records, rows->d_rows, int(p.stripes.size()), s.count, s.width, s.height,
                                                            erase, erase ? s.background : 0u, root.comm_stream), what));
}

// The most records a device can pack for a step: one per tile of its shard of every frame.
inline size_t record_capacity(const StepShape& s, const PeerPart& p) {
    return size_t(s.count) * p.stripes.size() * size_t((s.width + kifs::TILE_W - 1) / kifs::TILE_W);
}

// Posts the transfers of the step in `sl` and the root's scatter of what arrives.
int flush_slot(kifs_multi* m, StepSlot& sl) {
    if (!sl.used || sl.flushed) return KIFS_OK;
    const size_t n = m->dev.size();
    const size_t row_bytes = size_t(sl.width) * 4;
    const bool sparse = sl.gather == KIFS_GATHER_SPARSE;
    std::vector<Transfer> x(n);
    uint64_t records = 0, tiles = 0, payload = 0;
    for (size_t i = 1; i < n; ++i) {
        PeerPart& p = sl.part[i];
        p.n_records = 0, p.payload_bytes = 0;
        if (p.stripes.empty()) continue;
        if (sparse) {
            // the count was copied to pinned memory before `packed` was recorded
            if (!hip_ok(hipEventSynchronize(p.packed), "wait(packed)")) return KIFS_ERR_RUNTIME;
            const size_t capacity = record_capacity(sl, p);
            if (*p.h_count > capacity) return KIFS_ERR_RUNTIME;
            p.n_records = *p.h_count;
            p.payload_bytes = size_t(p.n_records) * KIFS_SPARSE_RECORD_BYTES;
            records += p.n_records;
            tiles += capacity;
        } else {
            p.payload_bytes = size_t(sl.count) * size_t(p.rows) * row_bytes;
        }
        x[i] = Transfer{sparse ? p.records : p.buf.shard, p.buf.recv, p.payload_bytes, p.packed};
        payload += p.payload_bytes;
    }
    int st = transfer_to_root(m, x, false);
    if (st != KIFS_OK) return st;
    m->stats.records_received += records;  // (counted once the transfers are posted: a failed flush that is
    m->stats.tiles_covered += tiles;       // tried again must not count twice)
    m->stats.bytes_received += payload;
    {   // the root moves what arrived to its rows of the frames
        const Device& root = m->dev[0];
        DeviceGuard g(root.id);
        for (size_t i = 1; i < n; ++i) {
            PeerPart& p = sl.part[i];
            if (!p.payload_bytes) continue;
            st = sparse ? unpack_records(root, sl, p, 0, "scatter of a received payload")
                        : unpack_dense(root, root.comm_stream, sl, p.buf.recv, size_t(p.rows) * row_bytes, p.stripes);
            if (st != KIFS_OK) return st;
        }
        if (!hip_ok(hipEventRecord(sl.gathered, root.comm_stream), "record(gathered)")) return KIFS_ERR_RUNTIME;
    }
    sl.flushed = true;
    sl.background_known = sparse && !sl.overwritten;
    if (m->have_pending && m->pending == sl.step) m->have_pending = false;
    return KIFS_OK;
}

// An older step that is still unflushed goes before `step`: the gather stream runs them in order.
int flush_older(kifs_multi* m, uint64_t step) {
    StepSlot& other = m->slot[(step + 1) % SLOTS];
    return other.used && other.step < step ? flush_slot(m, other) : int(KIFS_OK);
}

// Host-side completion of a slot's step (flushes it first if need be).
int complete_slot(kifs_multi* m, StepSlot& sl) {
    if (!sl.used) return KIFS_OK;
    int st = flush_slot(m, sl);
    if (st != KIFS_OK) return st;
    if (!hip_ok(hipEventSynchronize(sl.rendered), "wait(rendered)") || !hip_ok(hipEventSynchronize(sl.gathered), "wait(gathered)"))
        return KIFS_ERR_RUNTIME;
    sl.used = false;
    m->stats.steps += 1;
    return KIFS_OK;
}

int drain(kifs_multi* m) {
    // oldest first: a step's erase may depend on the step before it in the gather stream
    static_assert(SLOTS == 2, "drain orders two slots");
    const int first = m->slot[1].step < m->slot[0].step ? 1 : 0;
    int st = complete_slot(m, m->slot[first]);
    return st != KIFS_OK ? st : complete_slot(m, m->slot[1 - first]);
}

// Uniform changes apply to the steps submitted afterwards; steps in flight are completed first (their buffers and
// row partition belong to the old settings).
template <class Call>
int forward(kifs_multi* m, Call call) {
    if (!m) return KIFS_ERR_BAD_ARG;
    int st = drain(m);
    for (size_t i = 0; st == KIFS_OK && i < m->dev.size(); ++i) st = call(m->dev[i].ctx);
    return st;
}

// [frames, end) of what a step writes
inline const uint8_t* frames_end(const StepShape& s) {
    return s.frames + size_t(s.count - 1) * s.stride + size_t(s.height - 1) * s.pitch + size_t(s.width) * 4;
}

// Something is about to write [lo, hi) on the root: a slot whose frames overlap that range no longer knows that they
// hold the background outside its records -- its next submission must fill, whatever KIFS_MULTI_FRAMES_UNTOUCHED
// says (the other slot rendering into the same buffer, a lone kifs_multi_render into it, buffers that overlap).
void forget_background(kifs_multi* m, const StepSlot* except, const uint8_t* lo, const uint8_t* hi) {
    for (StepSlot& o : m->slot) {
        if (&o == except || !o.frames || o.count < 1) continue;
        if (lo < frames_end(o) && o.frames < hi) {
            o.background_known = false;
            o.overwritten = true;  // (also for a flush of that slot's step that is still to come)
        }
    }
}

void free_slot(kifs_multi* m, StepSlot& sl) {
    for (size_t i = 0; i < sl.part.size(); ++i) {
        PeerPart& p = sl.part[i];
        DeviceGuard g(m->dev[i].id);
        free_payload(p.buf, m->dev[0].id);
        if (p.records) (void)hipFree(p.records);
        if (p.d_count) (void)hipFree(p.d_count);
        if (p.h_count) (void)hipHostFree(p.h_count);
        if (p.packed) (void)hipEventDestroy(p.packed);
    }
    if (sl.rendered || sl.gathered) {
        DeviceGuard g(m->dev[0].id);
        if (sl.rendered) (void)hipEventDestroy(sl.rendered);
        if (sl.gathered) (void)hipEventDestroy(sl.gathered);
    }
    sl = StepSlot();
}

// A Device is filled and emptied as a unit -- but for its context, which comes first and goes last.
int open_device(Device& d, int id, int root_id) {
    int st = KIFS_OK;
    d.id = id;
    d.ctx = kifs_create(id, &st);
    if (!d.ctx) return st;
    DeviceGuard g(id);
    if (hipEventCreate(&d.ev0) != hipSuccess || hipEventCreate(&d.ev1) != hipSuccess) return KIFS_ERR_DEVICE_INIT;
    if (id != root_id) {  // direct xGMI access both ways; failure only means staged copies
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, id, root_id) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(root_id, 0);
        (void)hipGetLastError();
    }
    return KIFS_OK;
}

void close_device(Device& d, int root_id) {
    if (!d.ctx) return;  // (nothing else is made without it)
    DeviceGuard g(d.id);
    if (d.comm_stream) (void)hipStreamDestroy(d.comm_stream);
    free_payload(d.lone, root_id);
    if (d.ev0) (void)hipEventDestroy(d.ev0);
    if (d.ev1) (void)hipEventDestroy(d.ev1);
}

// ---- a submission, piece by piece.  The argument and size checks; `now` is the step they describe.
int check_step(kifs_multi* m, int count, const KifsCameraUniform* cameras, uint8_t* dev_frames, size_t frame_pitch,
               size_t frame_stride, int encode, StepShape* now) {
    if (!m || !cameras || !dev_frames || count < 1 || count > KIFS_MAX_BATCH) return KIFS_ERR_BAD_ARG;
    if (encode != KIFS_ENCODE_UNORM && encode != KIFS_ENCODE_SRGB) return KIFS_ERR_BAD_ARG;
    const Device& root = m->dev[0];
    if (!root.ctx->have_screen || !root.ctx->have_options) return KIFS_ERR_UNCONFIGURED;
    int w, h;
    int st = render_dims(root.ctx, &w, &h);
    if (st != KIFS_OK) return st;
    const size_t row_bytes = size_t(w) * 4;
    if (frame_pitch < row_bytes || ((frame_pitch | frame_stride) & 3u) || (reinterpret_cast<uintptr_t>(dev_frames) & 3u) ||
        (count > 1 && frame_stride < frame_pitch * size_t(h - 1) + row_bytes))
        return KIFS_ERR_BAD_SIZE;
    DeviceGuard g(root.id);
    if (!g.ok) return KIFS_ERR_RUNTIME;
    if (!is_device_pointer(dev_frames)) return KIFS_ERR_BAD_ARG;
    const float* bc = root.ctx->options.background_color;
    *now = StepShape{count, encode, m->gather, w, h, dev_frames, frame_pitch, frame_stride,
                     background_pixel(root.ctx, kifs::V3{bc[0], bc[1], bc[2]}, encode)};
    return KIFS_OK;
}

// May the frames be assumed to hold the background everywhere but under the slot's last records?  Decided from the
// slot's record of its previous step and the step that is about to take its place, nothing else.
bool erase_suffices(const kifs_multi* m, const StepSlot& sl, const StepShape& now, int flags) {
    if (now.gather != KIFS_GATHER_SPARSE || !(flags & KIFS_MULTI_FRAMES_UNTOUCHED) || !sl.background_known) return false;
    if (sl.part.size() != m->dev.size()) return false;
    for (size_t i = 0; i < sl.part.size(); ++i)
        if (sl.part[i].stripes != m->dev[i].stripes) return false;
    return sl.frames == now.frames && sl.pitch == now.pitch && sl.stride == now.stride && sl.count == now.count &&
           sl.encode == now.encode && sl.background == now.background && sl.width == now.width && sl.height == now.height &&
           sl.gather == now.gather;
}

// The root's gather stream: background under everybody else's rows of the frames of `now` -- an erase under the
// records the slot still holds of its previous step, or a fill of every such row.
int paint_background(kifs_multi* m, StepSlot& sl, const StepShape& now, bool erase_only) {
    const Device& root = m->dev[0];
    DeviceGuard g(root.id);
    if (erase_only) {
        int st = KIFS_OK;
        for (size_t i = 1; st == KIFS_OK && i < sl.part.size(); ++i)
            if (sl.part[i].n_records) st = unpack_records(root, now, sl.part[i], 1, "erase of the previous records");
        return st;
    }
    sl.peer_stripes.clear();
    for (size_t i = 1; i < m->dev.size(); ++i)
        sl.peer_stripes.insert(sl.peer_stripes.end(), m->dev[i].stripes.begin(), m->dev[i].stripes.end());
    std::sort(sl.peer_stripes.begin(), sl.peer_stripes.end());
    if (sl.peer_stripes.empty()) return KIFS_OK;
    const RowTable* rows = row_table(root.ctx, sl.peer_stripes.data(), int(sl.peer_stripes.size()), now.height);
    if (!rows) return KIFS_ERR_RUNTIME;
    return runtime_status(hip_ok(kifs::launch_fill_stripes(now.frames, now.pitch, now.stride, rows->d_rows, int(sl.peer_stripes.size()),
                                                           now.count, now.width, now.height, now.background, root.comm_stream),
                                 "fill under the other devices' rows"));
}

// One device's part of the step in `sl`: one launch for its shard of all the step's frames (the root: in place, then
// `rendered`), then its payload and `packed`.
int submit_device(kifs_multi* m, StepSlot& sl, size_t i, const KifsCameraUniform* cameras) {
    Device& d = m->dev[i];
    PeerPart& p = sl.part[i];
    const bool is_root = i == 0, sparse = sl.gather == KIFS_GATHER_SPARSE;
    hipStream_t stream = d.ctx->stream;
    p.stripes = d.stripes;
    p.rows = d.rows;
    p.n_records = 0, p.payload_bytes = 0;
    DeviceGuard g(d.id);
    if (!g.ok) return KIFS_ERR_RUNTIME;
    d.shard_ms = -1.0;
    if (p.stripes.empty()) return runtime_status(!is_root || hip_ok(hipEventRecord(sl.rendered, stream), "record(rendered)"));
    const size_t row_bytes = size_t(sl.width) * 4, shard_stride = size_t(p.rows) * row_bytes;
    if (is_root) {
        for (int f = 0; f < sl.count; ++f) m->outs_scratch[size_t(f)] = sl.frames + size_t(f) * sl.stride;
    } else {
        const size_t need = shard_stride * size_t(sl.count);
        const size_t record_bytes = record_capacity(sl, p) * KIFS_SPARSE_RECORD_BYTES;
        if (!make_event(p.packed)) return KIFS_ERR_RUNTIME;
        // buffers that grow are replaced while nothing reads them: the slot's previous step is complete, and its
        // completion includes the root's scatter, which follows the transfer in the gather stream
        if (!grow_shard(p.buf, need, "hipMalloc(step shards)")) return KIFS_ERR_RUNTIME;
        if (sparse) {
            if (!grow(p.records, p.records_bytes, record_bytes, "hipMalloc(step records)")) return KIFS_ERR_RUNTIME;
            if (!p.d_count && !hip_ok(hipMalloc(reinterpret_cast<void**>(&p.d_count), sizeof(uint32_t)), "hipMalloc(record count)"))
                return KIFS_ERR_RUNTIME;
            if (!p.h_count && !hip_ok(hipHostMalloc(reinterpret_cast<void**>(&p.h_count), sizeof(uint32_t), hipHostMallocDefault),
                                      "hipHostMalloc(record count)"))
                return KIFS_ERR_RUNTIME;
        }
        if (!grow_recv(p.buf, m->dev[0].id, sparse ? record_bytes : need, "hipMalloc(step receive)")) return KIFS_ERR_RUNTIME;
        for (int f = 0; f < sl.count; ++f) m->outs_scratch[size_t(f)] = p.buf.shard + size_t(f) * shard_stride;
    }
    if (!hip_ok(hipEventRecord(d.ev0, stream), "record(launch start)")) return KIFS_ERR_RUNTIME;
    int st = enqueue_batch(d.ctx, stream, sl.count, cameras, m->outs_scratch.data(), is_root ? sl.pitch : row_bytes, 0, sl.height,
                           sl.encode, p.stripes.data(), int(p.stripes.size()), is_root ? 1 : 0);
    if (st != KIFS_OK) return st;
    if (!hip_ok(hipEventRecord(d.ev1, stream), "record(launch stop)")) return KIFS_ERR_RUNTIME;
    if (is_root) return runtime_status(hip_ok(hipEventRecord(sl.rendered, stream), "record(rendered)"));
    if (sparse) {
        const RowTable* rows = row_table(d.ctx, p.stripes.data(), int(p.stripes.size()), sl.height);
        if (!rows) return KIFS_ERR_RUNTIME;
        if (!hip_ok(hipMemsetAsync(p.d_count, 0, sizeof(uint32_t), stream), "memset(record count)") ||
            !hip_ok(kifs::launch_pack_sparse(p.buf.shard, row_bytes, shard_stride, rows->d_rows, int(p.stripes.size()), sl.count,
                                             sl.width, sl.height, sl.background, reinterpret_cast<uint32_t*>(p.records), p.d_count,
                                             stream), "pack_sparse_kernel launch") ||
            !hip_ok(hipMemcpyAsync(p.h_count, p.d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream), "copy(record count)"))
            return KIFS_ERR_RUNTIME;
    }
    return runtime_status(hip_ok(hipEventRecord(p.packed, stream), "record(packed)"));
}

// A step that was only partly enqueued is no step: whatever was launched is waited for (it writes into the caller's
// frames and the slot's buffers), the slot is free again, the step number is not used up -- a later submit, wait or
// destroy must not flush record counts and events of a launch that never happened.
int abandon_step(kifs_multi* m, StepSlot& sl, int st) {
    for (Device& d : m->dev) {
        DeviceGuard g(d.id);
        (void)hipStreamSynchronize(d.ctx->stream);
    }
    DeviceGuard g(m->dev[0].id);
    (void)hipStreamSynchronize(m->dev[0].comm_stream);
    (void)hipGetLastError();
    sl.used = sl.flushed = sl.background_known = false;
    return st;
}

// The pipeline after the step in `sl` has been enqueued: the step before it is flushed -- its senders have had a
// whole submission to pack -- and this one becomes the pending one.
int advance_pipeline(kifs_multi* m, StepSlot& sl) {
    if (m->have_pending) {
        StepSlot& prev = m->slot[m->pending % SLOTS];
        int st = KIFS_OK;
        if (prev.used && prev.step == m->pending && (st = flush_slot(m, prev)) != KIFS_OK) return st;
        m->have_pending = false;
    }
    if (!sl.flushed) {
        m->have_pending = true;
        m->pending = sl.step;
    }
    return KIFS_OK;
}

// what device i sends in kifs_multi_comm_selftest
inline uint8_t selftest_byte(size_t k, size_t i) { return uint8_t((k * 131u + i * 29u + 7u) & 255u); }

}  // namespace

extern "C" {

void kifs_multi_destroy(kifs_multi* m) {
    if (!m) return;
    (void)drain(m);
    for (Device& d : m->dev) {
        if (!d.ctx) continue;
        DeviceGuard g(d.id);
        (void)hipStreamSynchronize(d.ctx->stream);
        if (d.comm_stream) (void)hipStreamSynchronize(d.comm_stream);
    }
    destroy_comms(m);
    for (StepSlot& sl : m->slot) free_slot(m, sl);
    for (Device& d : m->dev) close_device(d, m->dev[0].id);
    if (m->root_frame) {
        DeviceGuard g(m->dev[0].id);
        (void)hipFree(m->root_frame);
    }
    for (Device& d : m->dev) kifs_destroy(d.ctx);
    delete m;
}

kifs_multi* kifs_multi_create(const int* devices, int n, int* status) {
    auto fail = [&](int st, kifs_multi* m) -> kifs_multi* {
        if (status) *status = st;
        kifs_multi_destroy(m);
        return nullptr;
    };
    if (!devices || n <= 0 || n > 64) return fail(KIFS_ERR_BAD_ARG, nullptr);
    kifs_multi* m = new (std::nothrow) kifs_multi();
    if (!m) return fail(KIFS_ERR_DEVICE_INIT, nullptr);
    m->stats.gather = m->gather;
    m->dev.reserve(size_t(n));
    for (int i = 0; i < n; ++i) {
        m->dev.emplace_back();
        int st = open_device(m->dev.back(), devices[i], devices[0]);
        if (st != KIFS_OK) return fail(st, m);
    }
    if (status) *status = KIFS_OK;
    return m;
}

int kifs_multi_set_screen(kifs_multi* m, const KifsScreenUniform* s) { return forward(m, [=](kifs_ctx* c) { return kifs_set_screen(c, s); }); }
int kifs_multi_set_camera(kifs_multi* m, const KifsCameraUniform* s) { return forward(m, [=](kifs_ctx* c) { return kifs_set_camera(c, s); }); }
int kifs_multi_set_options(kifs_multi* m, const KifsOptionsUniform* s) { return forward(m, [=](kifs_ctx* c) { return kifs_set_options(c, s); }); }
int kifs_multi_set_iters(kifs_multi* m, int a, int b, int f) { return forward(m, [=](kifs_ctx* c) { return kifs_set_iters(c, a, b, f); }); }
int kifs_multi_set_extensions(kifs_multi* m, const KifsExtensions* e) { return forward(m, [=](kifs_ctx* c) { return kifs_set_extensions(c, e); }); }
int kifs_multi_set_supersampling(kifs_multi* m, int k) { return forward(m, [=](kifs_ctx* c) { return kifs_set_supersampling(c, k); }); }

int kifs_multi_set_weights(kifs_multi* m, const int* weights) {
    if (!m) return KIFS_ERR_BAD_ARG;
    long long total = 0;
    for (size_t i = 0; i < m->dev.size(); ++i) {
        const int w = weights ? weights[i] : 1;
        if (w < 0 || w > (1 << 20)) return KIFS_ERR_BAD_ARG;
        total += w;
    }
    if (total <= 0) return KIFS_ERR_BAD_ARG;
    int st = drain(m);
    if (st != KIFS_OK) return st;
    for (size_t i = 0; i < m->dev.size(); ++i) m->dev[i].weight = weights ? weights[i] : 1;
    m->stripes_height = -1;
    return KIFS_OK;
}

int kifs_multi_shard(kifs_multi* m, int i, int* device, int* n_stripes, int* rows) {
    if (!m || i < 0 || size_t(i) >= m->dev.size()) return KIFS_ERR_BAD_ARG;
    int w, h;
    if (!m->dev[0].ctx->have_screen) return KIFS_ERR_UNCONFIGURED;
    int st = frame_dims(m->dev[0].ctx, &w, &h);
    if (st != KIFS_OK || (st = multi_partition(m, h)) != KIFS_OK) return st;
    const Device& d = m->dev[size_t(i)];
    if (device) *device = d.id;
    if (n_stripes) *n_stripes = int(d.stripes.size());
    if (rows) *rows = d.rows;
    return KIFS_OK;
}

double kifs_multi_shard_ms(kifs_multi* m, int i) {
    if (!m || i < 0 || size_t(i) >= m->dev.size()) return -1.0;
    Device& d = m->dev[size_t(i)];
    // batched steps leave their launches' event pairs behind: resolved here, once they have completed
    if (d.shard_ms < 0.0 && d.ev0 && d.ev1) {
        DeviceGuard g(d.id);
        float ms = 0.0f;
        if (hipEventQuery(d.ev1) == hipSuccess && hipEventElapsedTime(&ms, d.ev0, d.ev1) == hipSuccess) d.shard_ms = double(ms);
        (void)hipGetLastError();
    }
    return d.shard_ms;
}

int kifs_multi_render(kifs_multi* m, uint8_t* out, size_t pitch, int encode) {
    if (!m || !out) return KIFS_ERR_BAD_ARG;
    Device& root = m->dev[0];
    if (!root.ctx->have_screen || !root.ctx->have_camera || !root.ctx->have_options) return KIFS_ERR_UNCONFIGURED;
    int w, h;
    int st = render_dims(root.ctx, &w, &h);
    if (st != KIFS_OK) return st;
    const size_t row_bytes = size_t(w) * 4;
    if (pitch < row_bytes || (pitch & 3u)) return KIFS_ERR_BAD_SIZE;
    // (batched steps in flight use the same contexts and streams)
    if ((st = drain(m)) != KIFS_OK || (st = multi_partition(m, h)) != KIFS_OK) return st;
    forget_background(m, nullptr, out, out + size_t(h - 1) * pitch + row_bytes);  // (a host pointer overlaps nothing)
    // the frame the shards are collected into: the caller's buffer if it is root-device memory
    uint8_t* frame = out;
    size_t fpitch = pitch;
    bool host_dst;
    {
        DeviceGuard g(root.id);
        host_dst = !is_device_pointer(out);
        if (host_dst) {
            if (!grow(m->root_frame, m->root_frame_bytes, row_bytes * size_t(h), "hipMalloc(multi frame)")) return KIFS_ERR_RUNTIME;
            frame = m->root_frame;
            fpitch = row_bytes;
        }
    }
    // 1. every device renders its shard: the root straight into the frame, the others into a packed buffer
    for (Device& d : m->dev) {
        const bool is_root = &d == &root;
        DeviceGuard g(d.id);
        uint8_t* dst = frame;
        size_t dpitch = fpitch;
        if (!is_root) {
            if (!grow_shard(d.lone, row_bytes * size_t(d.rows), "hipMalloc(shard)")) return KIFS_ERR_RUNTIME;
            dst = d.lone.shard;
            dpitch = row_bytes;
        }
        if (hipEventRecord(d.ev0, d.ctx->stream) != hipSuccess) return KIFS_ERR_RUNTIME;
        if (!d.stripes.empty()) {
            st = enqueue_batch(d.ctx, d.ctx->stream, 1, nullptr, &dst, dpitch, 0, h, encode, d.stripes.data(), int(d.stripes.size()),
                               is_root ? 1 : 0);
            if (st != KIFS_OK) return st;
        }
        if (hipEventRecord(d.ev1, d.ctx->stream) != hipSuccess) return KIFS_ERR_RUNTIME;
    }
    // 2. the root pulls each finished shard over xGMI and moves its stripes to their frame rows: a peer copy on its
    //    render stream, whatever the transport of the batched steps is
    {
        DeviceGuard g(root.id);
        hipStream_t rstream = root.ctx->stream;
        const StepShape one{1, encode, KIFS_GATHER_DENSE, w, h, frame, fpitch, 0, 0u};
        for (size_t i = 1; i < m->dev.size(); ++i) {
            Device& d = m->dev[i];
            if (d.stripes.empty()) continue;
            if (!grow_recv(d.lone, root.id, row_bytes * size_t(d.rows), "hipMalloc(received shard)")) return KIFS_ERR_RUNTIME;
            if (hipStreamWaitEvent(rstream, d.ev1, 0) != hipSuccess) return KIFS_ERR_RUNTIME;
            if (!hip_ok(hipMemcpyPeerAsync(d.lone.recv, root.id, d.lone.shard, d.id, row_bytes * size_t(d.rows), rstream),
                        "peer copy of a shard"))
                return KIFS_ERR_COMM;
            if ((st = unpack_dense(root, rstream, one, d.lone.recv, 0, d.stripes)) != KIFS_OK) return st;
        }
        if (host_dst &&
            !hip_ok(hipMemcpy2DAsync(out, pitch, frame, fpitch, row_bytes, size_t(h), hipMemcpyDeviceToHost, rstream), "frame to host"))
            return KIFS_ERR_RUNTIME;
        if (!hip_ok(hipStreamSynchronize(rstream), "multi sync")) return KIFS_ERR_RUNTIME;
    }
    for (Device& d : m->dev) {
        DeviceGuard g(d.id);
        if (hipStreamSynchronize(d.ctx->stream) != hipSuccess) return KIFS_ERR_RUNTIME;
        float ms = 0.0f;
        d.shard_ms = hipEventElapsedTime(&ms, d.ev0, d.ev1) == hipSuccess ? double(ms) : -1.0;
    }
    return KIFS_OK;
}

// ---- batched steps ---------------------------------------------------------------------------------------

int kifs_multi_set_gather(kifs_multi* m, int gather, int transport) {
    if (!m || (gather != KIFS_GATHER_SPARSE && gather != KIFS_GATHER_DENSE) ||
        (transport != KIFS_TRANSPORT_AUTO && transport != KIFS_TRANSPORT_RCCL && transport != KIFS_TRANSPORT_COPY))
        return KIFS_ERR_BAD_ARG;
    int st = drain(m);
    if (st != KIFS_OK) return st;
    m->gather = m->stats.gather = gather;
    if (transport != m->transport_wanted || (transport != KIFS_TRANSPORT_AUTO && transport != m->transport)) {
        // a different transport: communicators go, the next step (or the lines below) decides anew
        destroy_comms(m);
        m->transport_wanted = transport;
        m->transport = m->stats.transport = KIFS_TRANSPORT_AUTO;
    }
    for (StepSlot& sl : m->slot) sl.background_known = false;
    if (transport == KIFS_TRANSPORT_AUTO) return KIFS_OK;
    st = ensure_streams(m);  // an explicit transport is set up now, so that its failure is reported here
    return st != KIFS_OK ? st : ensure_transport(m);
}

int kifs_multi_render_batch_async(kifs_multi* m, int count, const KifsCameraUniform* cameras, uint8_t* dev_frames,
                                  size_t frame_pitch, size_t frame_stride, int encode, int flags, uint64_t* step_out) {
    StepShape now;
    int st = check_step(m, count, cameras, dev_frames, frame_pitch, frame_stride, encode, &now);
    if (st != KIFS_OK || (st = ensure_streams(m)) != KIFS_OK || (st = ensure_transport(m)) != KIFS_OK ||
        (st = multi_partition(m, now.height)) != KIFS_OK)
        return st;
    const size_t n = m->dev.size();
    const uint64_t step = m->next_step;
    StepSlot& sl = m->slot[step % SLOTS];
    // the slot's previous step (k - 2) ends here: its consumer has had it since the wait, or never asked
    if ((st = complete_slot(m, sl)) != KIFS_OK) return st;
    const bool erase_only = erase_suffices(m, sl, now, flags);
    // (that looked at this slot's own record of the buffer; the OTHER slot's record of any buffer this step writes
    // into is void from here on)
    forget_background(m, &sl, now.frames, frames_end(now));
    if (sl.part.size() != n) sl.part.resize(n);
    {
        DeviceGuard g(m->dev[0].id);
        if (!make_event(sl.rendered) || !make_event(sl.gathered)) return KIFS_ERR_RUNTIME;
    }
    if (now.gather == KIFS_GATHER_SPARSE && n > 1 && (st = paint_background(m, sl, now, erase_only)) != KIFS_OK) return st;
    static_cast<StepShape&>(sl) = now;
    sl.step = step;
    sl.used = true;
    sl.flushed = sl.background_known = sl.overwritten = false;
    m->outs_scratch.resize(size_t(count));
    for (size_t i = 0; st == KIFS_OK && i < n; ++i) st = submit_device(m, sl, i, cameras);
    if (st == KIFS_OK && n == 1) {  // nothing to gather
        DeviceGuard g(m->dev[0].id);
        if (hip_ok(hipEventRecord(sl.gathered, m->dev[0].comm_stream), "record(gathered)")) sl.flushed = true;
        else st = KIFS_ERR_RUNTIME;
    }
    if (st != KIFS_OK) return abandon_step(m, sl, st);
    m->next_step = step + 1;
    if (step_out) *step_out = step;
    return advance_pipeline(m, sl);
}

int kifs_multi_wait(kifs_multi* m, uint64_t step) {
    if (!m || step >= m->next_step) return KIFS_ERR_BAD_ARG;
    StepSlot& sl = m->slot[step % SLOTS];
    if (!sl.used || sl.step != step) return KIFS_OK;  // completed earlier (by a later submission or a wait)
    int st = flush_older(m, step);
    return st != KIFS_OK ? st : complete_slot(m, sl);
}

int kifs_multi_wait_all(kifs_multi* m) { return m ? drain(m) : KIFS_ERR_BAD_ARG; }

int kifs_multi_stream_wait(kifs_multi* m, uint64_t step, void* hip_stream) {
    if (!m || !hip_stream || step >= m->next_step) return KIFS_ERR_BAD_ARG;
    StepSlot& sl = m->slot[step % SLOTS];
    if (!sl.used || sl.step != step) return KIFS_OK;
    int st = flush_older(m, step);
    if (st != KIFS_OK || (st = flush_slot(m, sl)) != KIFS_OK) return st;
    DeviceGuard g(m->dev[0].id);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return runtime_status(hip_ok(hipStreamWaitEvent(s, sl.rendered, 0), "stream wait(rendered)") &&
                          hip_ok(hipStreamWaitEvent(s, sl.gathered, 0), "stream wait(gathered)"));
}

int kifs_multi_order_after(kifs_multi* m, void* producer_stream) {
    if (!m) return KIFS_ERR_BAD_ARG;
    int st = ensure_streams(m);
    if (st != KIFS_OK) return st;
    const Device& root = m->dev[0];
    // the root's render stream first (kifs_order_after records the context's ordering event on the producer's
    // stream), then the same event for the gather stream
    if ((st = kifs_order_after(root.ctx, nullptr, producer_stream)) != KIFS_OK) return st;
    if (root.ctx->stream == static_cast<hipStream_t>(producer_stream)) return KIFS_OK;
    DeviceGuard g(root.id);
    return runtime_status(hip_ok(hipStreamWaitEvent(root.comm_stream, root.ctx->ev_order, 0), "wait(multi order_after)"));
}

int kifs_multi_render_batch(kifs_multi* m, int count, const KifsCameraUniform* cameras, uint8_t* dev_frames,
                            size_t frame_pitch, size_t frame_stride, int encode) {
    uint64_t step = 0;
    int st = kifs_multi_render_batch_async(m, count, cameras, dev_frames, frame_pitch, frame_stride, encode, 0, &step);
    return st != KIFS_OK ? st : kifs_multi_wait(m, step);
}

int kifs_multi_stats(kifs_multi* m, KifsMultiStats* out, int reset) {
    if (!m || !out) return KIFS_ERR_BAD_ARG;
    *out = m->stats;
    if (reset) {
        m->stats.steps = 0;
        m->stats.records_received = 0;
        m->stats.tiles_covered = 0;
        m->stats.bytes_received = 0;
    }
    return KIFS_OK;
}

int kifs_multi_comm_selftest(kifs_multi* m, size_t bytes) {
    if (!m || bytes == 0 || bytes > (size_t(1) << 30)) return KIFS_ERR_BAD_ARG;
    int st = drain(m);
    if (st != KIFS_OK || (st = ensure_streams(m)) != KIFS_OK || (st = ensure_transport(m)) != KIFS_OK) return st;
    const size_t n = m->dev.size();
    const int root_id = m->dev[0].id;
    const bool self = n == 1;  // one device: the root sends to itself and receives from itself in one group
    std::vector<Payload> buf(n);  // what a step would send, for the length of this call
    std::vector<Transfer> x(n);
    std::vector<uint8_t> pattern(bytes), back(bytes);
    int rc = KIFS_OK;
    for (size_t i = self ? 0 : 1; i < n && rc == KIFS_OK; ++i) {
        for (size_t k = 0; k < bytes; ++k) pattern[k] = selftest_byte(k, i);
        {
            DeviceGuard g(m->dev[i].id);
            if (!grow_shard(buf[i], bytes, "hipMalloc(selftest)") ||
                !hip_ok(hipMemcpy(buf[i].shard, pattern.data(), bytes, hipMemcpyHostToDevice), "hipMemcpy(selftest)"))
                rc = KIFS_ERR_RUNTIME;
        }
        DeviceGuard g(root_id);
        if (rc == KIFS_OK && (!grow_recv(buf[i], root_id, bytes, "hipMalloc(selftest)") ||
                              !hip_ok(hipMemset(buf[i].recv, 0, bytes), "hipMemset(selftest)")))
            rc = KIFS_ERR_RUNTIME;
        x[i] = Transfer{buf[i].shard, buf[i].recv, bytes, nullptr};
    }
    if (rc == KIFS_OK) rc = transfer_to_root(m, x, self);
    if (rc == KIFS_OK) {
        for (Device& d : m->dev) {
            DeviceGuard g(d.id);
            if (!hip_ok(hipStreamSynchronize(d.comm_stream), "sync(selftest)")) rc = KIFS_ERR_COMM;
        }
    }
    for (size_t i = self ? 0 : 1; i < n && rc == KIFS_OK; ++i) {
        DeviceGuard g(root_id);
        if (!hip_ok(hipMemcpy(back.data(), x[i].dst, bytes, hipMemcpyDeviceToHost), "hipMemcpy(selftest back)")) {
            rc = KIFS_ERR_RUNTIME;
            break;
        }
        for (size_t k = 0; k < bytes && rc == KIFS_OK; ++k)
            if (back[k] != selftest_byte(k, i)) rc = KIFS_ERR_COMM;
    }
    for (size_t i = 0; i < n; ++i) {
        DeviceGuard g(m->dev[i].id);
        free_payload(buf[i], root_id);
    }
    return rc;
}

}  // extern "C"
