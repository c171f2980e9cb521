// storage.hip -- GraphStorage / FeatureStorage / MemoryPool for the MI355X build.
//
// Reference: SS/storage/graph_storage.cu:12-111 (pointer tables with P+1 slots, slot P = full
// CSR, slot d = GPU d's cached CSR; GraphCache), SS/storage/feature_storage.cu:18-90 (per-GPU
// seed/label arrays), SS/engine/server.cu:216-234 + SS/engine/ipc_service.cu:134-211 (buffers),
// SS/engine/server_imp.cuh:2-51 (alloc helpers).
//
// Layout decision for 288 GB HBM: the "host" tier pointers (full CSR, full feature table) are just
// device-dereferenceable pointers; the caller places them in HBM when they fit and in mapped
// pinned memory otherwise.  Nothing here assumes which.
#include "legion_core.h"
#include "reverse_rule.h"
#include <unistd.h>
#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

#include <cstring>
#include <cerrno>
#include <string>
#include <thread>
#include <sys/time.h>

#include "../trainer/vmm_map.h"        // vmm_map_chunks(): a range of this process built from another process's chunks (+ ipc_wire.h: the messages)

// ---- device helpers: logical device ids beyond the physical count map round-robin onto the
//      physical GPUs, so that clique striping (Kg > 1) can be exercised on a 1-GPU box ----------
static int lg_physical_count()
{
    static int n = -1;
    if (n < 0) {
        if (hipGetDeviceCount(&n) != hipSuccess || n < 1) {
            printf("legion_hip: no HIP device available -- this library has no CPU fallback\n");
            exit(EXIT_FAILURE);
        }
    }
    return n;
}

// One process per GPU (torchrun): the process's logical GPU 0 is physical GPU `base` (= LOCAL_RANK)
static int g_device_base = 0;
extern "C" void legion_set_device_base(int32_t base) { g_device_base = base < 0 ? 0 : base; }
extern "C" int32_t legion_get_device_base(void) { return g_device_base; }

static int g_local_only = -1;
extern "C" void legion_set_local_device(int32_t dev) { g_local_only = dev; }
bool lg_is_local(int32_t dev) { return g_local_only < 0 || dev == g_local_only; }

// physical device a logical GPU of this process runs on
int lg_physical_device(int32_t dev) { return (g_device_base + dev) % lg_physical_count(); }

extern "C" void SetGPUDevice(int32_t shard_id)
{
    HIP_CALL(hipSetDevice((g_device_base + shard_id) % lg_physical_count()));
}

extern "C" int32_t GetGPUDevice()
{
    int32_t dev_id = -1;
    HIP_CALL(hipGetDevice(&dev_id));
    return dev_id;
}

// ---- device memory whose pieces come from all over the HBM ----------------------------------------------------------------------------
// One contiguous VIRTUAL range backed by physical chunks that are created one by one and mapped in shuffled order (HIP virtual memory
// management).  Why ("where the lanes sit"): the last hop's gather writes a launch group's rows into the group's lanes; with
// the lanes in one hipMalloc'ed block -- one contiguous physical range -- it runs at 0.80 of the HBM peak, with the same block built from
// shuffled 2 MB ... 128 MB chunks at 0.87 (whole job 5.19 -> 5.57 G edges/s), better than what separate allocations get on a machine
// whose free memory happens to be fragmented (0.84-0.85) and independent of that luck.  Not exportable with hipIpcGetMemHandle and
// mapped for THIS device only; what another process or another GPU must reach is created exportable (below) and granted / served.
namespace {
struct ScatterLive {
    size_t bytes;
    std::vector<hipMemGenericAllocationHandle_t> chunks;
    std::vector<int> listeners;       // sockets of lg_scattered_serve threads (each thread takes its own out again when it ends)
    bool exportable = false;          // chunks created with a POSIX-file-descriptor handle type: only these can be exported / served
};
std::mutex g_scatter_mu;
std::map<void*, ScatterLive> g_scatter_live;
}
static void* alloc_scattered(int64_t num_bytes, int32_t chunk_mb, bool exportable);
extern "C" void* d_alloc_scattered(int64_t num_bytes, int32_t chunk_mb) { return alloc_scattered(num_bytes, chunk_mb, false); }
// ... whose chunks can be handed to another process as file descriptors (the server's lane arena: lg_scattered_export_fd)
extern "C" void* d_alloc_scattered_exportable(int64_t num_bytes, int32_t chunk_mb) { return alloc_scattered(num_bytes, chunk_mb, true); }
static void* alloc_scattered(int64_t num_bytes, int32_t chunk_mb, bool exportable)
{
    int dev = 0;
    HIP_CALL(hipGetDevice(&dev));
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = dev;
    if (exportable) prop.requestedHandleType = hipMemHandleTypePosixFileDescriptor;
    size_t g0 = 0;
    HIP_CALL(hipMemGetAllocationGranularity(&g0, &prop, hipMemAllocationGranularityRecommended));          // (4 KB on this stack)
    const size_t want = (size_t)(chunk_mb > 0 ? chunk_mb : 2) << 20;
    const size_t g = (want + g0 - 1) / g0 * g0;
    const size_t n = ((size_t)(num_bytes > 0 ? num_bytes : 16) + g - 1) / g;
    ScatterLive live;
    live.bytes = n * g;
    live.exportable = exportable;
    live.chunks.resize(n);
    for (size_t i = 0; i < n; i++) HIP_CALL(hipMemCreate(&live.chunks[i], g, &prop, 0));
    uint64_t r = 0x9E3779B97F4A7C15ull;
    for (size_t i = n - 1; i > 0; i--) {                                                       // Fisher-Yates, fixed seed
        r ^= r << 13; r ^= r >> 7; r ^= r << 17;
        std::swap(live.chunks[i], live.chunks[(size_t)(r % (uint64_t)(i + 1))]);
    }
    void* ptr = nullptr;
    HIP_CALL(hipMemAddressReserve(&ptr, n * g, 0, nullptr, 0));
    for (size_t i = 0; i < n; i++) HIP_CALL(hipMemMap((char*)ptr + i * g, g, 0, live.chunks[i], 0));
    hipMemAccessDesc acc = {};
    acc.location.type = hipMemLocationTypeDevice;
    acc.location.id = dev;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    HIP_CALL(hipMemSetAccess(ptr, n * g, &acc, 1));
    std::lock_guard<std::mutex> lk(g_scatter_mu);
    g_scatter_live[ptr] = std::move(live);
    return ptr;
}
// chunk size of a scattered allocation (0: `ptr` is not one) and its number of chunks, in mapping order
extern "C" int64_t lg_scattered_info(void* ptr, int32_t* n_chunks)
{
    std::lock_guard<std::mutex> lk(g_scatter_mu);
    auto it = g_scatter_live.find(ptr);
    if (it == g_scatter_live.end() || it->second.chunks.empty()) return 0;
    if (n_chunks) *n_chunks = (int32_t)it->second.chunks.size();
    return (int64_t)(it->second.bytes / it->second.chunks.size());
}
// a new file descriptor for chunk `index` of an exportable scattered allocation (the caller closes it), or -1.  The export runs
// under the registry's lock: d_free_scattered takes the allocation out of the registry under the same lock before it releases the
// chunks, so a handle is never exported while it is being released.
extern "C" int lg_scattered_export_fd(void* ptr, int32_t index)
{
    std::lock_guard<std::mutex> lk(g_scatter_mu);
    auto it = g_scatter_live.find(ptr);
    if (it == g_scatter_live.end() || !it->second.exportable || index < 0 || (size_t)index >= it->second.chunks.size()) return -1;
    int fd = -1;
    if (hipMemExportToShareableHandle(&fd, it->second.chunks[(size_t)index], hipMemHandleTypePosixFileDescriptor, 0) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return fd;
}
// 1 when `ptr` is a scattered allocation whose chunks can be exported (d_alloc_scattered_exportable)
extern "C" int32_t lg_scattered_exportable(void* ptr)
{
    std::lock_guard<std::mutex> lk(g_scatter_mu);
    auto it = g_scatter_live.find(ptr);
    return (it != g_scatter_live.end() && it->second.exportable) ? 1 : 0;
}
// ---- a scattered allocation reached from OTHER GPUs / processes -------------------------------------------------------------------
// (the server's lane arena handed to a trainer; since round 5 also the lane arenas owners push rows into, peer_gather = bulk: round 4
// kept those plain because hipIpcGetMemHandle cannot export memory made with hipMemCreate, and the bulk leg started 7 % behind what
// the shuffled placement is worth to the gathers.)
// Same process, other GPUs: the range is made accessible to those devices as well.
extern "C" int32_t lg_scattered_grant(void* ptr, const int32_t* logical_devs, int32_t n)
{
    size_t bytes = 0;
    {
        std::lock_guard<std::mutex> lk(g_scatter_mu);
        auto it = g_scatter_live.find(ptr);
        if (it == g_scatter_live.end()) return 0;
        bytes = it->second.bytes;
    }
    std::vector<hipMemAccessDesc> acc;
    for (int32_t i = 0; i < n; i++) {
        const int phys = lg_physical_device(logical_devs[i]);
        bool seen = false;
        for (const auto& a : acc) seen = seen || a.location.id == phys;
        if (seen) continue;
        hipMemAccessDesc d = {};
        d.location.type = hipMemLocationTypeDevice;
        d.location.id = phys;
        d.flags = hipMemAccessFlagsProtReadWrite;
        acc.push_back(d);
    }
    if (acc.empty()) return 1;
    const hipError_t e = hipMemSetAccess(ptr, bytes, acc.data(), acc.size());
    if (e != hipSuccess) {          // (the caller decides: a bulk leg without peer access to the arenas cannot run, everything else can)
        (void)hipGetLastError();
        printf("legion_hip: hipMemSetAccess for %d device(s) failed: '%s'\n", (int)acc.size(), hipGetErrorString(e));
        return 0;
    }
    return 1;
}

// Other processes: a detached thread hands the chunks' file descriptors (64 per SCM_RIGHTS message, in mapping order) to whoever
// connects to the abstract unix socket `name` -- if it is a process of the same user (SO_PEERCRED: a descriptor to device memory is a
// capability, and the abstract namespace has no file permissions).  `ptr` must be an EXPORTABLE scattered allocation.  The thread and
// its socket go when the allocation is freed (d_free_scattered shuts the socket down; the thread, woken by that, closes it).
extern "C" int32_t lg_scattered_serve(void* ptr, const char* name)
{
    int32_t n_chunks = 0;
    if (lg_scattered_info(ptr, &n_chunks) <= 0) return 0;
    if (!lg_scattered_exportable(ptr)) {
        printf("legion_hip: %s: the allocation was not created exportable (d_alloc_scattered_exportable): its chunks cannot be served\n", name);
        return 0;
    }
    const int ls = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
    if (ls < 0) return 0;
    sockaddr_un addr;
    const socklen_t len = wire_abstract_address(&addr, name);
    if (bind(ls, (sockaddr*)&addr, len) != 0 || listen(ls, 16) != 0) { close(ls); return 0; }
    {
        std::lock_guard<std::mutex> lk(g_scatter_mu);
        auto it = g_scatter_live.find(ptr);
        if (it == g_scatter_live.end()) { close(ls); return 0; }
        it->second.listeners.push_back(ls);
    }
    int hip_dev = 0;
    (void)hipGetDevice(&hip_dev);                      // (the caller's device: the allocation's)
    std::thread([ls, ptr, n_chunks, hip_dev]() {
        (void)hipSetDevice(hip_dev);
        for (;;) {
            const int c = accept4(ls, nullptr, nullptr, SOCK_CLOEXEC);
            if (c < 0) {
                // the allocation has been freed (d_free_scattered took it out of the registry, then shut the socket down): close and go.
                // Anything else -- EINTR, ECONNABORTED, EMFILE / ENFILE, ENOMEM ... -- is transient: a later peer must still be served.
                bool freed;
                {
                    std::lock_guard<std::mutex> lk(g_scatter_mu);
                    auto it = g_scatter_live.find(ptr);
                    freed = it == g_scatter_live.end() || std::find(it->second.listeners.begin(), it->second.listeners.end(), ls) == it->second.listeners.end();
                }
                if (freed) { close(ls); return; }
                if (errno != EINTR) usleep(2000);
                continue;
            }
            {   // a peer that connects and never reads must not block the only serving thread for ever
                timeval tv = {2, 0};
                (void)setsockopt(c, SOL_SOCKET, SO_SNDTIMEO, &tv, sizeof(tv));
            }
            {
                ucred cr;
                socklen_t cl = sizeof(cr);
                if (getsockopt(c, SOL_SOCKET, SO_PEERCRED, &cr, &cl) != 0 || cr.uid != geteuid()) {
                    printf("legion_hip: refused a request for device-memory descriptors from uid %d (pid %d)\n", (int)cr.uid, (int)cr.pid);
                    fflush(stdout);
                    close(c);
                    continue;
                }
            }
            bool ok = true;
            for (int32_t i0 = 0; i0 < n_chunks && ok; i0 += WIRE_FD_BATCH) {
                const int32_t n = std::min(WIRE_FD_BATCH, n_chunks - i0);
                int fds[WIRE_FD_BATCH];
                for (int32_t i = 0; i < n; i++) { fds[i] = lg_scattered_export_fd(ptr, i0 + i); ok = ok && fds[i] >= 0; }
                if (ok) ok = wire_send_fd_batch(c, fds, n) == 0;
                for (int32_t i = 0; i < n; i++) if (fds[i] >= 0) close(fds[i]);
            }
            close(c);
        }
    }).detach();
    return 1;
}

// ... and the other side: connect to `name`, receive n_chunks descriptors, import and map them back to back, accessible to THIS
// process's current device.  Returns the base address or null (why: printed).  lg_scattered_unmap_remote gives everything back.
struct RemoteMap { size_t chunk_bytes; int32_t n_chunks; };
static std::map<void*, RemoteMap> g_remote_maps;
extern "C" void* lg_scattered_map_remote(const char* name, int32_t n_chunks, int64_t chunk_bytes)
{
    if (n_chunks <= 0 || chunk_bytes <= 0) return nullptr;
    int dev = 0;
    HIP_CALL(hipGetDevice(&dev));
    const char* why = "";
    void* base = vmm_map_chunks(name, n_chunks, chunk_bytes, dev, &why);
    if (base == nullptr) {
        printf("legion_hip: mapping %d chunks of %s failed (%s)\n", n_chunks, name, why);
        return nullptr;
    }
    std::lock_guard<std::mutex> lk(g_scatter_mu);
    g_remote_maps[base] = RemoteMap{(size_t)chunk_bytes, n_chunks};
    return base;
}
extern "C" void lg_scattered_unmap_remote(void* base)
{
    RemoteMap m;
    {
        std::lock_guard<std::mutex> lk(g_scatter_mu);
        auto it = g_remote_maps.find(base);
        if (it == g_remote_maps.end()) return;
        m = it->second;
        g_remote_maps.erase(it);
    }
    vmm_unmap_chunks(base, m.n_chunks, m.n_chunks, (long long)m.chunk_bytes);
}

static bool d_free_scattered(void* ptr)
{
    ScatterLive live;
    {
        std::lock_guard<std::mutex> lk(g_scatter_mu);
        auto it = g_scatter_live.find(ptr);
        if (it == g_scatter_live.end()) return false;
        live = std::move(it->second);
        g_scatter_live.erase(it);
    }
    for (int ls : live.listeners) shutdown(ls, SHUT_RDWR);      // wakes the serving thread out of accept(); it finds the allocation gone and closes the socket itself
    HIP_CALL(hipMemUnmap(ptr, live.bytes));
    HIP_CALL(hipMemAddressFree(ptr, live.bytes));
    for (auto h : live.chunks) HIP_CALL(hipMemRelease(h));
    return true;
}

// ---- a pipeline's lane-PRIVATE arrays (slot arrays, claim lists, frontier headers ...) from one block of shuffled chunks as well
//      (PoolSource, legion_core.h): carved in the order they are asked for, never freed one by one ----------------------------------
PrivateBlock* lg_private_block_create(int64_t bytes, int32_t scatter_mb)
{
    PrivateBlock* b = new PrivateBlock();
    b->base = (char*)(scatter_mb > 0 ? d_alloc_scattered(bytes, scatter_mb) : nullptr);
    if (b->base == nullptr) HIP_CALL(hipMalloc((void**)&b->base, (size_t)bytes));
    b->bytes = bytes;
    return b;
}
void lg_private_block_destroy(PrivateBlock* b)
{
    if (!b) return;
    d_free_space(b->base);
    delete b;
}
void* lg_private_take(PrivateBlock* b, int64_t bytes)
{
    if (b == nullptr) return d_alloc_space(bytes);
    const int64_t need = pool_round(bytes);
    if (b->used + need > b->bytes) {
        printf("legion_hip: private block of %lld bytes is too small (%lld in use, %lld more asked for)\n", (long long)b->bytes,
               (long long)b->used, (long long)need);
        exit(EXIT_FAILURE);
    }
    void* p = b->base + b->used;
    b->used += need;
    return p;
}

extern "C" void* d_alloc_space(int64_t num_bytes)
{
    void* ret = nullptr;
    HIP_CALL(hipMalloc(&ret, num_bytes > 0 ? (size_t)num_bytes : 16));
    return ret;
}

static bool lg_ipc_try_export(void* handle64, void* dev_ptr, int attempts, hipError_t* last)
{
    for (int attempt = 0; attempt < attempts; attempt++) {
        *last = hipIpcGetMemHandle((hipIpcMemHandle_t*)handle64, dev_ptr);
        if (*last == hipSuccess) return true;
        (void)hipGetLastError();
        usleep(25000);
    }
    return false;
}

static void lg_ipc_diagnose(void* dev_ptr, hipError_t e, const char* file, int line)
{
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    const hipError_t pe = hipPointerGetAttributes(&at, dev_ptr);
    (void)hipGetLastError();
    const char* legacy = getenv("HSA_ENABLE_IPC_MODE_LEGACY");
    printf("HIP failure %s:%d: '%s' (hipIpcGetMemHandle of %p; attributes %s: device %d, type %d, base %p; "
           "HSA_ENABLE_IPC_MODE_LEGACY=%s)\n", file, line, hipGetErrorString(e), dev_ptr, hipGetErrorString(pe), at.device,
           (int)at.type, at.devicePointer, legacy ? legacy : "(unset)");
    fflush(stdout);
}

void lg_ipc_export(void* handle64, void* dev_ptr, const char* file, int line)
{
    hipError_t e = hipSuccess;
    if (lg_ipc_try_export(handle64, dev_ptr, 20, &e)) return;
    lg_ipc_diagnose(dev_ptr, e, file, line);
    exit(EXIT_FAILURE);
}

// A fresh device buffer together with its IPC handle.  About one server start in a hundred on this pool (ROCm 7.2, dmabuf
// IPC) finds EVERY small block of the process unexportable ('invalid argument', pointer attributes fine, mode variable
// set) while other starts export the same sizes without trouble -- small allocations are fragments of a shared runtime
// block there.  A block that keeps failing is set aside (not freed: the allocator would hand it out again) and a block of
// its own (>= 2 MiB, not a fragment) is tried instead.
void* lg_alloc_exported(int64_t num_bytes, void* handle64, const char* file, int line)
{
    hipError_t e = hipSuccess;
    void* p = nullptr;
    for (int block = 0; block < 4; block++) {
        const int64_t bytes = block == 0 ? num_bytes : std::max<int64_t>(num_bytes, ((int64_t)2 << 20) * block + 4096);
        p = d_alloc_space(bytes);
        if (lg_ipc_try_export(handle64, p, block == 0 ? 3 : 6, &e)) {
            if (block > 0) { printf("legion_hip: IPC export succeeded with a block of %lld bytes\n", (long long)bytes); fflush(stdout); }
            return p;
        }
        lg_ipc_diagnose(p, e, file, line);
    }
    exit(EXIT_FAILURE);
}

extern "C" void d_free_space(void* d_ptr)
{
    if (d_ptr && !d_free_scattered(d_ptr)) HIP_CALL(hipFree(d_ptr));
}

extern "C" void* host_alloc_space(int64_t num_bytes)
{
    void* host_ptr = nullptr;
    void* ret = nullptr;
    HIP_CALL(hipHostMalloc(&host_ptr, num_bytes > 0 ? (size_t)num_bytes : 16, hipHostMallocMapped));
    HIP_CALL(hipHostGetDevicePointer(&ret, host_ptr, 0));
    return ret;
}

// spill-over tier: mapped pinned host memory the GPU dereferences over PCIe (SS/engine/server_imp.cuh:41-51,
// storage_management.cu:106-107,161); returns the device-side pointer, *host_ptr_out the host-side one
extern "C" void* legion_host_alloc(int64_t num_bytes, void** host_ptr_out)
{
    void* host_ptr = nullptr;
    void* dev_ptr = nullptr;
    HIP_CALL(hipHostMalloc(&host_ptr, num_bytes > 0 ? (size_t)num_bytes : 16, hipHostMallocMapped));
    HIP_CALL(hipHostGetDevicePointer(&dev_ptr, host_ptr, 0));
    if (host_ptr_out) *host_ptr_out = host_ptr;
    return dev_ptr;
}

extern "C" void legion_host_free(void* host_ptr)
{
    if (host_ptr) HIP_CALL(hipHostFree(host_ptr));
}

extern "C" int32_t legion_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" const char* legion_version(void) { return "legion-hip 0.1 (gfx950)"; }

// =============================================================================================
class CompleteGraphStorage : public GraphStorage {
public:
    void Build(BuildInfo* info) override
    {
        partition_count_ = info->partition_count;
        node_num_ = info->total_num_nodes;
        edge_num_ = info->total_edge_num;
        csr_node_index_cpu_ = info->csr_node_index;
        csr_dst_node_ids_cpu_ = info->csr_dst_node_ids;
        csr_node_index_.assign(partition_count_, nullptr);
        csr_dst_node_ids_.assign(partition_count_, nullptr);
        h_index_tab_.assign(partition_count_, std::vector<int64_t*>(partition_count_ + 1, nullptr));
        h_dst_tab_.assign(partition_count_, std::vector<int32_t*>(partition_count_ + 1, nullptr));
        row_hdr_.assign(partition_count_, nullptr);
        topo_index_.assign(partition_count_, nullptr);
        topo_col_.assign(partition_count_, nullptr);
        csr_dst_x_.assign(partition_count_, nullptr);
        colx_full_.assign(partition_count_, nullptr);
        for (int32_t i = 0; i < partition_count_; i++) {
            if (!lg_is_local(i)) continue;
            SetGPUDevice(i);
            csr_node_index_[i] = (int64_t**)d_alloc_space((partition_count_ + 1) * sizeof(int64_t*));
            csr_dst_node_ids_[i] = (int32_t**)d_alloc_space((partition_count_ + 1) * sizeof(int32_t*));
            // every GPU can reach the full CSR through slot P (the reference initialises only
            // GPU 0's table before GraphCache copies it around, graph_storage.cu:62,77-80)
            h_index_tab_[i][partition_count_] = csr_node_index_cpu_;
            h_dst_tab_[i][partition_count_] = csr_dst_node_ids_cpu_;
            Upload(i);
            // per-vertex row headers: everything starts in the full CSR (slot P)
            row_hdr_[i] = (RowHdr*)d_alloc_space((int64_t)node_num_ * sizeof(RowHdr));
            lg::init_row_headers(nullptr, row_hdr_[i], csr_node_index_cpu_, node_num_, partition_count_);
            HIP_CALL(hipDeviceSynchronize());
        }
    }

    // SS/storage/graph_storage.cu:76-111: GPU i of clique Ki caches vertices QT[row*Kg + i]
    void GraphCache(int32_t* QT, int32_t Ki, int32_t Kg, int32_t capacity) override
    {
        GraphCacheBuildLocal(QT, Ki, Kg, capacity);
        GraphCacheLink(QT, Ki, Kg, capacity);
    }

    void GraphCacheBuildLocal(int32_t* QT, int32_t Ki, int32_t Kg, int32_t capacity) override
    {
        for (int32_t i = 0; i < Kg; i++) {
            const int32_t dev = Ki * Kg + i;
            if (!lg_is_local(dev)) continue;
            SetGPUDevice(dev);
            // a new fill: headers that an earlier fill pointed into ITS cached CSR go back to the full CSR first (a vertex
            // cached then and not now kept a row offset into arrays the pointer table no longer names)
            lg::init_row_headers(nullptr, row_hdr_[dev], csr_node_index_cpu_, node_num_, partition_count_);
            HIP_CALL(hipDeviceSynchronize());
            int64_t* neighbor_count = (int64_t*)d_alloc_space((int64_t)capacity * sizeof(int64_t));
            lg::topo_neighbor_count(nullptr, QT, Kg, i, capacity, node_num_, csr_node_index_cpu_, neighbor_count);
            int64_t* d_csr_node_index = (int64_t*)d_alloc_space(((int64_t)capacity + 1) * sizeof(int64_t));
            HIP_CALL(hipMemset(d_csr_node_index, 0, ((size_t)capacity + 1) * sizeof(int64_t)));
            if (capacity > 0) lg::inclusive_scan_i64(nullptr, neighbor_count, d_csr_node_index + 1, capacity);
            int64_t cached_edges = 0;
            HIP_CALL(hipMemcpy(&cached_edges, d_csr_node_index + capacity, sizeof(int64_t), hipMemcpyDeviceToHost));
            int32_t* d_csr_dst_node_ids = (int32_t*)d_alloc_space(cached_edges * sizeof(int32_t));
            lg::topo_fill_up(nullptr, QT, Kg, i, capacity, node_num_, csr_node_index_cpu_,
                             csr_dst_node_ids_cpu_, d_csr_node_index, d_csr_dst_node_ids);
            HIP_CALL(hipDeviceSynchronize());
            d_free_space(neighbor_count);
            owned_.push_back(d_csr_node_index);
            owned_.push_back(d_csr_dst_node_ids);
            topo_index_[dev] = d_csr_node_index;
            topo_col_[dev] = d_csr_dst_node_ids;
        }
    }

    void GraphCacheLink(int32_t* QT, int32_t Ki, int32_t Kg, int32_t capacity) override
    {
        for (int32_t j = 0; j < Kg; j++) {                // every LOCAL member of the clique ...
            const int32_t member = Ki * Kg + j;
            if (!lg_is_local(member)) continue;
            SetGPUDevice(member);
            for (int32_t i = 0; i < Kg; i++) {            // ... sees every member's cached CSR it knows of
                const int32_t dev = Ki * Kg + i;
                if (topo_index_[dev] == nullptr) continue;
                h_index_tab_[member][dev] = topo_index_[dev];
                h_dst_tab_[member][dev] = topo_col_[dev];
                // resolve the vertices that member caches to its CSR (reads its indptr: a peer load when
                // the member is another GPU)
                lg::cache_row_headers(nullptr, row_hdr_[member], QT, Kg, i, capacity, node_num_, topo_index_[dev], dev);
                HIP_CALL(hipDeviceSynchronize());
            }
            Upload(member);
        }
    }

    void SetPeerCSR(int32_t dev, int64_t* csr_node_index, int32_t* csr_dst_node_ids) override
    {
        topo_index_[dev] = csr_node_index;
        topo_col_[dev] = csr_dst_node_ids;
    }
    int64_t* CachedCSRIndex(int32_t dev) const override { return topo_index_[dev]; }
    int32_t* CachedCSRDst(int32_t dev) const override { return topo_col_[dev]; }

    // column slots (legion_core.h): {neighbour id, node_map[neighbour]} pairs of the FULL column array, for GPU dev
    void BuildColumnSlots(int32_t dev, const int32_t* node_map, uint64_t stamp) override
    {
        if (dev < 0 || dev >= partition_count_ || !lg_is_local(dev)) return;
        DropColumnSlots(dev);
        if ((int32_t)colx_stamp_.size() < partition_count_) colx_stamp_.assign(partition_count_, 0);
        const int32_t mode = lg::tuning().col_slots;
        if (mode == 0 || node_map == nullptr || edge_num_ <= 0) return;
        SetGPUDevice(dev);
        const int64_t bytes = edge_num_ * 8;
        if (mode < 0) {
            hipPointerAttribute_t at;
            memset(&at, 0, sizeof(at));
            if (hipPointerGetAttributes(&at, csr_dst_node_ids_cpu_) != hipSuccess || at.type != hipMemoryTypeDevice) {
                (void)hipGetLastError();
                return;                       // column array in (pinned) host memory: the spill-over configuration keeps HBM free
            }
            // What is free NOW is what the full tables, the caches and the maps left (FillUp has run); the lanes of the launch
            // groups come afterwards and size themselves to what remains (bench.py, GPURunner::CreateGroups).  The copy is worth
            // 3-7 % of the whole job (the gather stops fetching a 128-byte line of node_map per row), so it is taken whenever it
            // fits half of the free HBM and leaves 24 GB for the lanes -- uk-union's 44 GB copy beside 160 GB of tables on a
            // 288 GB part (round 3 declined it: a flat quarter of the free memory)
            size_t free_b = 0, total_b = 0;
            HIP_CALL(hipMemGetInfo(&free_b, &total_b));
            if (bytes > (int64_t)(free_b / 2) || (int64_t)free_b - bytes < ((int64_t)24 << 30)) return;
        }
        colx_full_[dev] = (int32_t*)d_alloc_space(bytes);
        lg::build_column_slots(nullptr, csr_dst_node_ids_cpu_, node_map, colx_full_[dev], edge_num_);
        std::vector<int32_t*> tab(partition_count_ + 1, nullptr);
        tab[partition_count_] = colx_full_[dev];
        csr_dst_x_[dev] = (int32_t**)d_alloc_space((partition_count_ + 1) * sizeof(int32_t*));
        HIP_CALL(hipMemcpy(csr_dst_x_[dev], tab.data(), tab.size() * sizeof(int32_t*), hipMemcpyHostToDevice));
        HIP_CALL(hipDeviceSynchronize());
        colx_stamp_[dev] = stamp;
    }
    uint64_t ColumnSlotsStamp(int32_t dev) const override
    {
        return (dev >= 0 && dev < (int32_t)colx_stamp_.size() && dev < (int32_t)csr_dst_x_.size() && csr_dst_x_[dev] != nullptr) ? colx_stamp_[dev] : 0;
    }
    void DropColumnSlots(int32_t dev) override
    {
        if (dev < 0 || dev >= (int32_t)csr_dst_x_.size() || csr_dst_x_[dev] == nullptr) return;
        SetGPUDevice(dev);
        HIP_CALL(hipDeviceSynchronize());
        d_free_space(csr_dst_x_[dev]);
        d_free_space(colx_full_[dev]);
        csr_dst_x_[dev] = nullptr;
        colx_full_[dev] = nullptr;
        if (dev < (int32_t)colx_stamp_.size()) colx_stamp_[dev] = 0;
    }
    int32_t** GetCSRXMatrix(int32_t part_id) const override { return csr_dst_x_.empty() ? nullptr : csr_dst_x_[part_id]; }
    const int32_t* GetColumnSlotsFull(int32_t part_id) const override { return colx_full_.empty() ? nullptr : colx_full_[part_id]; }

    // weighted sampling (legion_core.h): the prefix-sum table over the full column array, built on the device current at the call
    int32_t SetEdgeWeights(hipStream_t s, const float* w) override
    {
        if (w == nullptr || weighted_used_) return -1;
        if (edge_cdf_ == nullptr) {
            HIP_CALL(hipGetDevice(&edge_cdf_dev_));
            edge_cdf_ = (float*)d_alloc_space((edge_num_ > 0 ? edge_num_ : 1) * (int64_t)sizeof(float));
            cdf_long_cap_ = (int32_t)lg::lg_weights_long_rows_cap(edge_num_);
            cdf_long_rows_ = (int32_t*)d_alloc_space(((int64_t)cdf_long_cap_ + 1) * sizeof(int32_t));
        }
        if (edge_num_ > 0) lg::build_edge_cdf(s, csr_node_index_cpu_, node_num_, w, edge_cdf_, cdf_long_rows_, cdf_long_cap_);
        return 0;
    }
    const float* EdgeCdf() const override { return edge_cdf_; }
    void MarkWeightedUsed() override { weighted_used_ = true; }

    // sorted rows (legion_core.h): two counts on the current device, read back once and remembered
    int32_t CheckRowsSorted(hipStream_t s) override
    {
        if (rows_sorted_ >= 0) return rows_sorted_;
        unsigned long long h[2] = {0, 0};
        if (edge_num_ > 1) {
            unsigned long long* d = (unsigned long long*)d_alloc_space(2 * sizeof(unsigned long long));
            HIP_CALL(hipMemsetAsync(d, 0, 2 * sizeof(unsigned long long), s));
            lg::launch_row_inversion_counts(s, csr_node_index_cpu_, csr_dst_node_ids_cpu_, node_num_, edge_num_, d);
            HIP_CALL(hipMemcpyAsync(h, d, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
            HIP_CALL(hipStreamSynchronize(s));
            d_free_space(d);
        }
        rows_sorted_ = h[0] == h[1] ? 1 : 0;
        return rows_sorted_;
    }
    int32_t RowsSorted() const override { return rows_sorted_; }

    // the reverse CSR (legion_core.h): built once on the current device, owned here
    int32_t BuildReverse(hipStream_t s) override
    {
        if (rev_edges_ >= 0) return 0;
        HIP_CALL(hipGetDevice(&rev_dev_));
        rev_edges_ = lg::build_reverse_csr(s, csr_node_index_cpu_, csr_dst_node_ids_cpu_, node_num_, edge_num_, &rev_indptr_, &rev_col_, &rev_eid_);
        return 0;
    }
    int64_t ReverseCSR(const int64_t** rindptr, const int32_t** rcol, const int64_t** reid) const override
    {
        const bool built = rev_edges_ >= 0;
        if (rindptr) *rindptr = built ? rev_indptr_ : nullptr;
        if (rcol) *rcol = built ? rev_col_ : nullptr;
        if (reid) *reid = built ? rev_eid_ : nullptr;
        return built ? rev_edges_ : -1;
    }

    void Finalize() override
    {
        if (rev_edges_ >= 0) {
            SetGPUDevice(rev_dev_);
            HIP_CALL(hipDeviceSynchronize());
            d_free_space(rev_indptr_);
            d_free_space(rev_col_);
            d_free_space(rev_eid_);
            rev_indptr_ = rev_eid_ = nullptr;
            rev_col_ = nullptr;
            rev_edges_ = -1;
        }
        if (edge_cdf_ != nullptr) {
            SetGPUDevice(edge_cdf_dev_);
            HIP_CALL(hipDeviceSynchronize());
            d_free_space(edge_cdf_);
            d_free_space(cdf_long_rows_);
            edge_cdf_ = nullptr;
            cdf_long_rows_ = nullptr;
        }
        for (int32_t i = 0; i < (int32_t)csr_dst_x_.size(); i++) DropColumnSlots(i);
        for (void* p : owned_) d_free_space(p);
        owned_.clear();
        for (RowHdr* p : row_hdr_) d_free_space(p);
        row_hdr_.clear();
        for (int32_t i = 0; i < partition_count_; i++) {
            if (!lg_is_local(i)) continue;
            d_free_space(csr_node_index_[i]);
            d_free_space(csr_dst_node_ids_[i]);
        }
        csr_node_index_.clear();
        csr_dst_node_ids_.clear();
    }

    int32_t GetPartitionCount() const override { return partition_count_; }
    int64_t** GetCSRNodeIndex(int32_t part_id) const override { return csr_node_index_[part_id]; }
    int32_t** GetCSRNodeMatrix(int32_t part_id) const override { return csr_dst_node_ids_[part_id]; }
    int64_t* GetCSRNodeIndexCPU() const override { return csr_node_index_cpu_; }
    int32_t* GetCSRNodeMatrixCPU() const override { return csr_dst_node_ids_cpu_; }
    int32_t NodeNum() const override { return node_num_; }
    int64_t EdgeNum() const override { return edge_num_; }
    const RowHdr* GetRowHeaders(int32_t part_id) const override { return row_hdr_[part_id]; }

private:
    void Upload(int32_t dev)
    {
        SetGPUDevice(dev);
        HIP_CALL(hipMemcpy(csr_node_index_[dev], h_index_tab_[dev].data(),
                           (partition_count_ + 1) * sizeof(int64_t*), hipMemcpyHostToDevice));
        HIP_CALL(hipMemcpy(csr_dst_node_ids_[dev], h_dst_tab_[dev].data(),
                           (partition_count_ + 1) * sizeof(int32_t*), hipMemcpyHostToDevice));
    }

    int32_t partition_count_ = 0;
    int32_t node_num_ = 0;
    int64_t edge_num_ = 0;
    std::vector<int64_t**> csr_node_index_;
    std::vector<int32_t**> csr_dst_node_ids_;
    std::vector<std::vector<int64_t*>> h_index_tab_;
    std::vector<std::vector<int32_t*>> h_dst_tab_;
    int64_t* csr_node_index_cpu_ = nullptr;
    int32_t* csr_dst_node_ids_cpu_ = nullptr;
    std::vector<void*> owned_;
    std::vector<RowHdr*> row_hdr_;
    std::vector<int64_t*> topo_index_;   // [P] cached CSR of each GPU (local build or peer pointer)
    std::vector<int32_t*> topo_col_;
    std::vector<int32_t**> csr_dst_x_;   // [P] device tables of pair arrays (column slots), null until built
    std::vector<int32_t*> colx_full_;    // [P] this GPU's {id, feature-cache slot} copy of the full column array
    std::vector<uint64_t> colx_stamp_;   // [P] (cache uid, fill generation) the pairs were built from
    float* edge_cdf_ = nullptr;          // [E] per-row prefix sums of the sanitised edge weights, or null (SetEdgeWeights)
    int32_t* cdf_long_rows_ = nullptr;   // scratch of its build: {count, rows longer than a wave scans}
    int32_t cdf_long_cap_ = 0;
    int edge_cdf_dev_ = 0;
    int32_t rows_sorted_ = -1;           // CheckRowsSorted's answer, -1 before the first check
    bool weighted_used_ = false;         // a weighted hop has been enqueued against this graph: the table stays as it is
    int64_t* rev_indptr_ = nullptr;      // [N + 1] the reverse CSR (BuildReverse), null before it
    int32_t* rev_col_ = nullptr;         // [E']
    int64_t* rev_eid_ = nullptr;         // [E']
    int64_t rev_edges_ = -1;             // E', -1 before the build
    int rev_dev_ = 0;
};

extern "C" GraphStorage* NewCompleteGraphStorage() { return new CompleteGraphStorage(); }

// =============================================================================================
class CompleteFeatureStorage : public FeatureStorage {
public:
    ~CompleteFeatureStorage() override
    {
        if (owned_host_ != nullptr) legion_host_free(owned_host_);
        else if (owned_dev_ != nullptr) d_free_space(owned_dev_);
    }

    void Build(BuildInfo* info, int /*in_memory_mode*/) override
    {
        Configure(info->partition_count, info->total_num_nodes, info->float_feature_len,
                  info->host_float_feature);
        dtype_ = info->feature_dtype;
        for (int32_t p = 0; p < partition_count_; p++) {
            if (p < (int32_t)info->training_set_ids.size())
                SetIds(p, TRAINMODE, info->training_set_ids[p].data(), info->training_labels[p].data(),
                       (int32_t)info->training_set_ids[p].size());
            if (p < (int32_t)info->validation_set_ids.size())
                SetIds(p, VALIDMODE, info->validation_set_ids[p].data(), info->validation_labels[p].data(),
                       (int32_t)info->validation_set_ids[p].size());
            if (p < (int32_t)info->testing_set_ids.size())
                SetIds(p, TESTMODE, info->testing_set_ids[p].data(), info->testing_labels[p].data(),
                       (int32_t)info->testing_set_ids[p].size());
        }
    }

    void Configure(int32_t partition_count, int32_t total_num_nodes, int32_t float_feature_len,
                   float* all_float_feature)
    {
        partition_count_ = partition_count;
        total_num_nodes_ = total_num_nodes;
        float_feature_len_ = float_feature_len;
        float_feature_ = all_float_feature;
        for (int m = 0; m < 3; m++) {
            ids_[m].assign(partition_count, nullptr);
            labels_[m].assign(partition_count, nullptr);
            size_[m].assign(partition_count, 0);
        }
    }

    void SetIds(int32_t dev_id, int32_t mode, const int32_t* host_ids, const int32_t* host_labels,
                int32_t count) override
    {
        SetGPUDevice(dev_id);
        d_free_space(ids_[mode][dev_id]);
        d_free_space(labels_[mode][dev_id]);
        ids_[mode][dev_id] = (int32_t*)d_alloc_space((int64_t)count * sizeof(int32_t));
        labels_[mode][dev_id] = (int32_t*)d_alloc_space((int64_t)count * sizeof(int32_t));
        if (count > 0) {
            HIP_CALL(hipMemcpy(ids_[mode][dev_id], host_ids, (size_t)count * 4, hipMemcpyHostToDevice));
            if (host_labels)
                HIP_CALL(hipMemcpy(labels_[mode][dev_id], host_labels, (size_t)count * 4, hipMemcpyHostToDevice))
            else
                HIP_CALL(hipMemset(labels_[mode][dev_id], 0, (size_t)count * 4));   // v2: labels are all 0 (F7)
        }
        size_[mode][dev_id] = count;
    }

    void Finalize() override
    {
        for (int m = 0; m < 3; m++)
            for (size_t p = 0; p < ids_[m].size(); p++) {
                d_free_space(ids_[m][p]);
                d_free_space(labels_[m][p]);
                ids_[m][p] = labels_[m][p] = nullptr;
            }
    }

    int32_t* GetTrainingSetIds(int32_t p) const override { return ids_[TRAINMODE][p]; }
    int32_t* GetValidationSetIds(int32_t p) const override { return ids_[VALIDMODE][p]; }
    int32_t* GetTestingSetIds(int32_t p) const override { return ids_[TESTMODE][p]; }
    int32_t* GetTrainingLabels(int32_t p) const override { return labels_[TRAINMODE][p]; }
    int32_t* GetValidationLabels(int32_t p) const override { return labels_[VALIDMODE][p]; }
    int32_t* GetTestingLabels(int32_t p) const override { return labels_[TESTMODE][p]; }
    int32_t TrainingSetSize(int32_t p) const override { return size_[TRAINMODE][p]; }
    int32_t ValidationSetSize(int32_t p) const override { return size_[VALIDMODE][p]; }
    int32_t TestingSetSize(int32_t p) const override { return size_[TESTMODE][p]; }
    int32_t TotalNodeNum() const override { return total_num_nodes_; }
    float* GetAllFloatFeature() const override { return float_feature_; }
    int32_t GetFloatFeatureLen() const override { return float_feature_len_; }
    int32_t FeatureDtype() const override { return dtype_; }

    // a bf16 copy of the float32 table `src` that this storage owns (legion_feature_create_ex): HBM, or mapped pinned host memory
    // under LEGION_TABLE_PLACEMENT=pinned; converted in place, so there is never a second float32 copy
    void ConvertTable(const float* src)
    {
        dtype_ = LEGION_FEATURE_BF16;
        const int32_t P = lg_feature_pitch(dtype_, float_feature_len_);
        const int64_t bytes = (int64_t)total_num_nodes_ * lg_feature_row_bytes(dtype_, float_feature_len_);
        lg::tuning_refresh();             // (LEGION_TABLE_PLACEMENT as it is now)
        if (lg::tuning().table_placement == 1) owned_dev_ = legion_host_alloc(bytes, &owned_host_);
        else owned_dev_ = d_alloc_space(bytes > 0 ? bytes : 16);
        if (src != nullptr) {
            lg::convert_f32_to_bf16(nullptr, src, total_num_nodes_, float_feature_len_, P, (uint16_t*)owned_dev_);
            HIP_CALL(hipDeviceSynchronize());
        } else {
            HIP_CALL(hipMemset(owned_dev_, 0, bytes > 0 ? (size_t)bytes : 16));
        }
        float_feature_ = (float*)owned_dev_;
    }

private:
    int32_t partition_count_ = 0, total_num_nodes_ = 0, float_feature_len_ = 0;
    float* float_feature_ = nullptr;
    int32_t dtype_ = LEGION_FEATURE_F32;
    void* owned_dev_ = nullptr;       // the bf16 table ConvertTable made (device-side address), and its host side when pinned
    void* owned_host_ = nullptr;
    std::vector<int32_t*> ids_[3], labels_[3];
    std::vector<int32_t> size_[3];
};

extern "C" FeatureStorage* NewCompleteFeatureStorage() { return new CompleteFeatureStorage(); }

// =============================================================================================
LanePtrs MemoryPool::HostLane(int32_t pipe) const
{
    LanePtrs h;
    memset(&h, 0, sizeof(h));
    h.sampled_ids = sampled_ids_[pipe];
    h.labels = labels_[pipe];
    h.agg_src_ids = agg_src_ids_;
    h.agg_dst_ids = agg_dst_ids_;
    h.agg_src_off = agg_src_off_[pipe];
    h.agg_dst_off = agg_dst_off_[pipe];
    h.tmp_part_ind = tmp_part_ind_;
    h.err_flag = err_dev;
    h.counter_mirror = counter_mirror_dev;
    h.claim_pairs = claim_pairs;
    h.run_off = run_off;
    h.claim_cnt = claim_cnt;
    h.claim_cap = claim_cap;
    h.ids_cap = num_ids;
    h.lds_buckets = 1 << lds_bucket_bits;
    h.known_pairs = known_pairs;
    h.known_cnt = known_cnt;
    h.known_cap = known_cap;
    h.node_counter = node_counter_[pipe];
    h.edge_counter = edge_counter_[pipe];
    h.slot_dst = slot_dst;
    h.slot_pos = slot_pos;
    h.slot_fs = slot_fs;
    h.node_slot = node_slot;
    h.max_slots = max_slots;
    h.tile_state = tile_state;
    h.hop_scratch = hop_scratch;
    h.fh_edge = fh_edge;
    h.cache_search_buffer = cache_search_buffer_;
    h.float_features = float_features_[pipe];
    int64_t rows = feature_rows < num_ids ? feature_rows : num_ids;
    h.feature_rows = (int32_t)rows;
    h.slot_pick = slot_pick;
    h.agg_edge_ids = agg_edge_ids;
    return h;
}

const LanePtrs* MemoryPool::DeviceLane()
{
    if (lanes_dirty_ || d_lanes_ == nullptr || uploaded_rows_ != feature_rows) {
        SetGPUDevice(dev_id);
        if (d_lanes_ == nullptr) d_lanes_ = (LanePtrs*)d_alloc_space((int64_t)pipeline_depth_ * sizeof(LanePtrs));
        std::vector<LanePtrs> h(pipeline_depth_);
        for (int32_t i = 0; i < pipeline_depth_; i++) h[i] = HostLane(i);
        HIP_CALL(hipMemcpy(d_lanes_, h.data(), h.size() * sizeof(LanePtrs), hipMemcpyHostToDevice));
        lanes_dirty_ = false;
        uploaded_rows_ = feature_rows;
    }
    return d_lanes_ + current_pipe_;
}

// one private array of the pool (pool_plan.h) takes `p`: the one list of which member is which (null: the array is gone)
static void pool_set_array(MemoryPool* mp, PoolArray what, void* p)
{
    switch (what) {
        case PA_CACHE_SEARCH: mp->SetCacheSearchBuffer((int32_t*)p); break;
        case PA_CLAIM_PAIRS: mp->claim_pairs = (unsigned long long*)p; break;
        case PA_CLAIM_CNT: mp->claim_cnt = (int32_t*)p; break;
        case PA_RUN_OFF: mp->run_off = (int32_t*)p; break;
        case PA_KNOWN_PAIRS: mp->known_pairs = (unsigned long long*)p; break;
        case PA_KNOWN_CNT: mp->known_cnt = (int32_t*)p; break;
        case PA_AGG_SRC_IDS: mp->SetAggSrcId((int32_t*)p); break;
        case PA_AGG_DST_IDS: mp->SetAggDstId((int32_t*)p); break;
        case PA_TMP_PART_IND: mp->SetTmpPartIdx((char*)p); break;
        case PA_TMP_PART_OFF: mp->SetTmpPartOff((int32_t*)p); break;
        case PA_SLOT_DST: mp->slot_dst = (int32_t*)p; break;
        case PA_SLOT_POS: mp->slot_pos = (int32_t*)p; break;
        case PA_SLOT_FS: mp->slot_fs = (int32_t*)p; break;
        case PA_NODE_SLOT: mp->node_slot = (int32_t*)p; break;
        case PA_TILE_STATE: mp->tile_state = (unsigned long long*)p; break;
        case PA_FH_EDGE: mp->fh_edge = (RowHdr*)p; break;
        case PA_HOP_SCRATCH: mp->hop_scratch = (int32_t*)p; break;
        case PA_COUNT: break;
    }
}

void MemoryPool::Finalize()
{
    SetGPUDevice(dev_id);
    d_free_space(d_lanes_);
    d_lanes_ = nullptr;
    for (size_t i = 0; i < private_arrays.size(); i++) {       // (carved ones go with their block)
        if (!private_carved) d_free_space(private_arrays[i]);
        pool_set_array(this, private_plan.entries[i].what, nullptr);
    }
    private_arrays.clear();
    if (err_host) HIP_CALL(hipHostFree(err_host));
    err_host = err_dev = nullptr;
    d_free_space(slot_pick);
    d_free_space(agg_edge_ids);
    slot_pick = nullptr;
    agg_edge_ids = nullptr;
    if (owns_buffers) {
        for (int i = 0; i < pipeline_depth_; i++) {
            d_free_space(float_features_[i]);
            d_free_space(labels_[i]);
            d_free_space(node_counter_[i]);
            d_free_space(edge_counter_[i]);
            d_free_space(sampled_ids_[i]);
            d_free_space(agg_src_off_[i]);
            d_free_space(agg_dst_off_[i]);
            float_features_[i] = nullptr;
            labels_[i] = node_counter_[i] = edge_counter_[i] = sampled_ids_[i] = nullptr;
            agg_src_off_[i] = agg_dst_off_[i] = nullptr;
        }
    }
}

PoolPrivatePlan lg_pool_private_plan(const PoolShape& shape, const PoolSource& source)
{
    const LegionTuning tune = lg::tuning();
    return pool_private_plan(shape, source.claims_hint, tune.lds_small_buckets, tune.lds_claim_cap, tune.lds_known_cap, tune.col_slots);
}

// server-private scratch of one GPU: SS/engine/server.cu:216-234 plus the compaction scratch
void lg_pool_alloc_private(MemoryPool* mp, int32_t dev_id, int32_t total_num_nodes, int32_t batch_size,
                           const int32_t* fanout, int32_t hop_num, int32_t float_feature_len, const PoolSource& source)
{
    SetGPUDevice(dev_id);
    lg::tuning_refresh();
    const PoolShape shape = pool_shape(batch_size, fanout, hop_num);
    if (shape.over_limit) {
        printf("legion_hip: batch %d with this fan-out needs %lld slots / %lld ids; the limit is 2^31\n", batch_size, (long long)shape.max_slots,
               (long long)shape.num_ids);
        exit(EXIT_FAILURE);
    }
    mp->max_new = shape.max_new;
    mp->max_fanout = shape.max_fanout;
    mp->dev_id = dev_id;
    mp->num_ids = (int32_t)shape.num_ids;
    mp->max_slots = (int32_t)shape.max_slots;
    mp->total_num_nodes = total_num_nodes;
    mp->batch_size = batch_size;
    mp->float_feature_len = float_feature_len;
    mp->source = source;
    // first touches (legion_core.h): one claim list and one known list per hash bucket, sized by the plan (sample_plan.h; PreSC's
    // maxima when the creator passed them on, PoolSource::claims_hint)
    const PoolPrivatePlan plan = mp->private_plan = lg_pool_private_plan(shape, source);
    mp->lds_bucket_bits = plan.sample.bucket_bits;
    mp->last_hop_claims_hint = source.claims_hint[0];
    mp->claim_cap = plan.sample.claim_cap;
    mp->known_cap = plan.sample.known_cap;
    mp->private_carved = source.priv != nullptr;
    for (int32_t i = 0; i < plan.n; i++) {
        const PoolPrivatePlan::Entry& e = plan.entries[i];
        void* p = lg_private_take(source.priv, e.bytes);
        mp->private_arrays.push_back(p);
        pool_set_array(mp, e.what, p);
        switch (e.what) {
            case PA_CLAIM_CNT: case PA_KNOWN_CNT: case PA_TILE_STATE: case PA_HOP_SCRATCH:
                HIP_CALL(hipMemset(p, 0, (size_t)e.bytes));
                break;
            case PA_SLOT_FS: case PA_NODE_SLOT:       // nothing carried yet
                lg::fill_value_i32(nullptr, (int32_t*)p, LG_FS_UNKNOWN, e.bytes / 4);
                break;
            default: break;
        }
    }
    if (mp->node_slot != nullptr) HIP_CALL(hipDeviceSynchronize());
    {   // host-visible error word (kernels OR LG_ERR_* into it; reading it costs the host nothing)
        void* h = nullptr;
        void* dptr = nullptr;
        HIP_CALL(hipHostMalloc(&h, 64, hipHostMallocMapped));
        memset(h, 0, 64);
        HIP_CALL(hipHostGetDevicePointer(&dptr, h, 0));
        mp->err_host = (int32_t*)h;
        mp->err_dev = (int32_t*)dptr;
    }
}

// edge-id mode: the per-slot picks and the per-edge ids, sized like slot_dst and agg_src_ids.  Plain allocations of the pool even
// where its trainer-visible arrays live in a lane arena (the arena's layout and the wire do not change)
void lg_pool_alloc_edge_ids(MemoryPool* mp)
{
    if (mp->slot_pick != nullptr && mp->agg_edge_ids != nullptr) return;
    SetGPUDevice(mp->dev_id);
    mp->slot_pick = (int32_t*)d_alloc_space((int64_t)mp->max_slots * sizeof(int32_t));
    mp->agg_edge_ids = (int64_t*)d_alloc_space((int64_t)mp->num_ids * sizeof(int64_t));
    HIP_CALL(hipMemset(mp->agg_edge_ids, 0xff, (size_t)mp->num_ids * sizeof(int64_t)));      // -1: no edge yet
}

// ---- C API ----------------------------------------------------------------------------------
extern "C" LegionGraphStorage* legion_graph_create(int32_t partition_count, int32_t node_num,
                                                   int64_t edge_num, const int64_t* csr_node_index,
                                                   const int32_t* csr_dst_node_ids)
{
    BuildInfo info;
    info.partition_count = partition_count;
    info.total_num_nodes = node_num;
    info.total_edge_num = edge_num;
    info.csr_node_index = const_cast<int64_t*>(csr_node_index);
    info.csr_dst_node_ids = const_cast<int32_t*>(csr_dst_node_ids);
    GraphStorage* g = NewCompleteGraphStorage();
    g->Build(&info);
    return reinterpret_cast<LegionGraphStorage*>(g);
}

// 1 when logical GPU dev samples from the {neighbour id, feature-cache slot} copy of the column array (column slots)
extern "C" int32_t legion_graph_column_slots(const LegionGraphStorage* g_, int32_t dev)
{
    const GraphStorage* g = reinterpret_cast<const GraphStorage*>(g_);
    return (g && dev >= 0 && dev < g->GetPartitionCount() && g->GetCSRXMatrix(dev) != nullptr) ? 1 : 0;
}

// the cached CSR GPU dev holds after a fill (GraphStorage::GraphCache, SS/storage/graph_storage.cu:76-111): device pointers to
// int64 index[capacity + 1] and int32 dst[index[capacity]], or nulls before any fill (introspection for the parity tests)
extern "C" void legion_graph_cached_csr(const LegionGraphStorage* g_, int32_t dev, const int64_t** index_out, const int32_t** dst_out)
{
    const GraphStorage* g = reinterpret_cast<const GraphStorage*>(g_);
    const bool ok = g && dev >= 0 && dev < g->GetPartitionCount();
    if (index_out) *index_out = ok ? g->CachedCSRIndex(dev) : nullptr;
    if (dst_out) *dst_out = ok ? g->CachedCSRDst(dev) : nullptr;
}

// weighted sampling: the per-row prefix-sum table from the caller's float32 w[E] (aligned with the full column array), built on
// `stream` on the current device; replaced by a later call, refused once a weighted hop has been enqueued against the graph
extern "C" int32_t legion_graph_set_edge_weights(LegionGraphStorage* g_, legion_stream_t stream, const float* w_devptr)
{
    GraphStorage* g = reinterpret_cast<GraphStorage*>(g_);
    if (!g || !w_devptr) return -1;
    return g->SetEdgeWeights(static_cast<hipStream_t>(stream), w_devptr);
}

extern "C" const float* legion_graph_edge_cdf(const LegionGraphStorage* g_)
{
    const GraphStorage* g = reinterpret_cast<const GraphStorage*>(g_);
    return g ? g->EdgeCdf() : nullptr;
}

// are the full CSR's rows sorted?  counted on `stream` once (it synchronises that stream), remembered in the graph
extern "C" int32_t legion_graph_check_rows_sorted(LegionGraphStorage* g_, legion_stream_t stream)
{
    GraphStorage* g = reinterpret_cast<GraphStorage*>(g_);
    return g ? g->CheckRowsSorted(static_cast<hipStream_t>(stream)) : -1;
}

// the reverse CSR: built once on `stream` on the current device (set-up: it synchronises that stream), owned by the graph
extern "C" int32_t legion_graph_build_reverse(LegionGraphStorage* g_, legion_stream_t stream)
{
    GraphStorage* g = reinterpret_cast<GraphStorage*>(g_);
    if (reverse_refusal(g != nullptr, g ? g->NodeNum() : 0) != ReverseRefusal::Ok) return -1;
    return g->BuildReverse(static_cast<hipStream_t>(stream));
}

extern "C" int64_t legion_graph_reverse_csr(const LegionGraphStorage* g_, const int64_t** rindptr, const int32_t** rcol, const int64_t** reid)
{
    const GraphStorage* g = reinterpret_cast<const GraphStorage*>(g_);
    if (g) return g->ReverseCSR(rindptr, rcol, reid);
    if (rindptr) *rindptr = nullptr;
    if (rcol) *rcol = nullptr;
    if (reid) *reid = nullptr;
    return -1;
}

extern "C" void legion_graph_destroy(LegionGraphStorage* g_)
{
    GraphStorage* g = reinterpret_cast<GraphStorage*>(g_);
    if (!g) return;
    g->Finalize();
    delete g;
}

extern "C" LegionFeatureStorage* legion_feature_create(int32_t partition_count, int32_t total_num_nodes,
                                                       int32_t float_feature_len,
                                                       const float* all_float_feature)
{
    CompleteFeatureStorage* f = new CompleteFeatureStorage();
    f->Configure(partition_count, total_num_nodes, float_feature_len, const_cast<float*>(all_float_feature));
    return reinterpret_cast<LegionFeatureStorage*>(static_cast<FeatureStorage*>(f));
}

extern "C" LegionFeatureStorage* legion_feature_create_ex(int32_t partition_count, int32_t total_num_nodes, int32_t float_feature_len,
                                                          int32_t feature_dtype, const float* all_float_feature)
{
    if (feature_dtype == LEGION_FEATURE_F32)
        return legion_feature_create(partition_count, total_num_nodes, float_feature_len, all_float_feature);
    if (feature_dtype != LEGION_FEATURE_BF16) {
        printf("legion_feature_create_ex: unknown feature dtype %d\n", feature_dtype);
        return nullptr;
    }
    CompleteFeatureStorage* f = new CompleteFeatureStorage();
    f->Configure(partition_count, total_num_nodes, float_feature_len, nullptr);
    f->ConvertTable(all_float_feature);
    return reinterpret_cast<LegionFeatureStorage*>(static_cast<FeatureStorage*>(f));
}

extern "C" int32_t legion_feature_dtype(const LegionFeatureStorage* f_)
{
    const FeatureStorage* f = reinterpret_cast<const FeatureStorage*>(f_);
    return f ? f->FeatureDtype() : LEGION_FEATURE_F32;
}

extern "C" int64_t legion_feature_row_bytes(const LegionFeatureStorage* f_)
{
    const FeatureStorage* f = reinterpret_cast<const FeatureStorage*>(f_);
    return f ? lg_feature_row_bytes(f->FeatureDtype(), f->GetFloatFeatureLen()) : 0;
}

extern "C" const void* legion_feature_table(const LegionFeatureStorage* f_)
{
    const FeatureStorage* f = reinterpret_cast<const FeatureStorage*>(f_);
    return f ? f->GetAllFloatFeature() : nullptr;
}

extern "C" void legion_convert_f32_to_bf16(legion_stream_t stream, const float* src, int64_t rows, int32_t D, uint16_t* dst)
{
    lg::convert_f32_to_bf16(static_cast<hipStream_t>(stream), src, rows, D, lg_feature_pitch(LEGION_FEATURE_BF16, D), dst);
}

extern "C" void legion_feature_set_ids(LegionFeatureStorage* f_, int32_t dev_id, int32_t mode,
                                       const int32_t* host_ids, const int32_t* host_labels, int32_t count)
{
    FeatureStorage* f = reinterpret_cast<FeatureStorage*>(f_);
    if (!f) { printf("invalid feature storage ptr\n"); return; }
    if (mode < 0 || mode > 2) { printf("invalid mode: %d\n", mode); return; }
    f->SetIds(dev_id, mode, host_ids, host_labels, count);
}

extern "C" void legion_feature_destroy(LegionFeatureStorage* f_)
{
    FeatureStorage* f = reinterpret_cast<FeatureStorage*>(f_);
    if (!f) return;
    f->Finalize();
    delete f;
}

// ---- output arena (legion_core.h PoolArena) ---------------------------------------------------
static void* arena_take(PoolArena* a, int64_t bytes)
{
    const int64_t need = (bytes + 255) & ~(int64_t)255;
    if (a->used + need > a->bytes) {
        printf("legion_hip: lane arena of %lld bytes is too small (%lld in use, %lld more asked for)\n", (long long)a->bytes,
               (long long)a->used, (long long)need);
        exit(EXIT_FAILURE);
    }
    void* p = a->base + a->used;
    a->used += need;
    return p;
}

MemoryPool* lg_pool_create(int32_t dev_id, int32_t total_num_nodes, int32_t batch_size, const int32_t* fanout, int32_t hop_num,
                           int32_t float_feature_len, int32_t pipeline_depth, const PoolSource& source)
{
    if (pipeline_depth < 1) pipeline_depth = 1;
    MemoryPool* mp = new MemoryPool(pipeline_depth);
    lg_pool_alloc_private(mp, dev_id, total_num_nodes, batch_size, fanout, hop_num, float_feature_len, source);
    PoolArena* arena = source.arena;
    const bool in_arena = arena != nullptr && pipeline_depth == 1;
    mp->owns_buffers = !in_arena;
    mp->arena_backed = in_arena;
    auto take = [&](int64_t bytes) { return in_arena ? arena_take(arena, bytes) : d_alloc_space(bytes); };
    if (in_arena && arena->mirror_dev != nullptr && arena->mirror_used < arena->mirror_lanes) {
        mp->counter_mirror_dev = arena->mirror_dev + 32 * (int64_t)arena->mirror_used;
        mp->counter_mirror_host = arena->mirror_host + 32 * (int64_t)arena->mirror_used;
        arena->mirror_used++;
    }
    for (int i = 0; i < pipeline_depth; i++) {            // ipc_service.cu:134-161 without the handles
        mp->SetSampledIds((int32_t*)take((int64_t)mp->num_ids * 4), i);
        mp->SetLabels((int32_t*)take((int64_t)batch_size * 4), i);
        mp->SetAggSrcOf((int32_t*)take((int64_t)mp->num_ids * 4), i);
        mp->SetAggDstOf((int32_t*)take((int64_t)mp->num_ids * 4), i);
        mp->SetNodeCounter((int32_t*)take(16 * 4), i);
        mp->SetEdgeCounter((int32_t*)take(16 * 4), i);
        mp->SetCurrentPipe(i);
        HIP_CALL(hipMemset(mp->GetNodeCounter(), 0, 64));
        HIP_CALL(hipMemset(mp->GetEdgeCounter(), 0, 64));
    }
    mp->SetCurrentPipe(0);
    return mp;
}

extern "C" LegionMemoryPool* legion_pool_create(int32_t dev_id, int32_t total_num_nodes, int32_t batch_size,
                                                const int32_t* fanout, int32_t hop_num,
                                                int32_t float_feature_len, int32_t pipeline_depth)
{
    return reinterpret_cast<LegionMemoryPool*>(lg_pool_create(dev_id, total_num_nodes, batch_size, fanout, hop_num, float_feature_len,
                                                              pipeline_depth, PoolSource()));
}

extern "C" void legion_pool_alloc_features(LegionMemoryPool* p_, int64_t rows)
{
    MemoryPool* mp = reinterpret_cast<MemoryPool*>(p_);
    if (!mp) { printf("invalid memorypool ptr\n"); return; }
    SetGPUDevice(mp->dev_id);
    const int32_t cur = mp->GetCurrentPipe();
    const int64_t row_bytes = (int64_t)mp->float_feature_len * lg_feature_out_bytes(mp->feature_out_dtype);
    mp->features_allocated = true;
    for (int i = 0; i < mp->PipelineDepth(); i++) {
        mp->SetCurrentPipe(i);
        if (mp->arena_backed) {           // (once per pool: the arena is sized for exactly one feature buffer per lane)
            mp->SetFloatFeatures((float*)arena_take(mp->source.arena, rows * row_bytes), i);
            continue;
        }
        d_free_space(mp->GetFloatFeatures());
        mp->SetFloatFeatures((float*)d_alloc_space(rows * row_bytes), i);
    }
    mp->SetCurrentPipe(cur);
    mp->feature_rows = rows;
}

// dtype of the rows the pool's gathers write (LEGION_FEATURE_*); only before the pool's first legion_pool_alloc_features
extern "C" int32_t legion_pool_set_feature_out_dtype(LegionMemoryPool* p_, int32_t dtype)
{
    MemoryPool* mp = reinterpret_cast<MemoryPool*>(p_);
    if (!mp || (dtype != LEGION_FEATURE_F32 && dtype != LEGION_FEATURE_BF16) || mp->features_allocated) return -1;
    mp->feature_out_dtype = dtype;
    return 0;
}

extern "C" int32_t legion_pool_feature_out_dtype(const LegionMemoryPool* p_)
{
    const MemoryPool* mp = reinterpret_cast<const MemoryPool*>(p_);
    return mp ? mp->feature_out_dtype : -1;
}

// The pool's sampling modes (sample_mode.h; include/legion_hip.h says what each means).  Only before the pool samples a hop.  Turning
// edge ids on allocates their two arrays, which stay until the pool goes; a change of edge_ids also changes the lane descriptor.
// Weighted mode allocates nothing: the table travels with the launch (HopParams)
bool lg_pool_try_set_mode(MemoryPool* mp, const SampleMode& mode, bool check_only)
{
    if (!mp || mp->sample_used || sample_mode_refusal(mode, mp->max_fanout) != SampleRefusal::Ok) return false;
    if (check_only) return true;
    const bool lane_changes = mode.edge_ids != mp->mode.edge_ids;
    if (mode.edge_ids) lg_pool_alloc_edge_ids(mp);
    mp->mode = mode;
    if (lane_changes) {
        mp->lanes_epoch++;                 // (lane groups made before this re-upload their copy of the lane: operators.hip)
        mp->InvalidateDeviceLanes();
    }
    return true;
}

// the pool's mode with one field changed, handed to lg_pool_try_set_mode
static int32_t pool_set_mode_field(LegionMemoryPool* p_, int32_t SampleMode::*field, int32_t value)
{
    MemoryPool* mp = reinterpret_cast<MemoryPool*>(p_);
    if (!mp) return -1;
    SampleMode mode = mp->mode;
    mode.*field = value;
    return lg_pool_try_set_mode(mp, mode) ? 0 : -1;
}
static int32_t pool_mode_field(const LegionMemoryPool* p_, int32_t SampleMode::*field)
{
    const MemoryPool* mp = reinterpret_cast<const MemoryPool*>(p_);
    return mp ? mp->mode.*field : -1;
}

extern "C" int32_t legion_pool_set_sample_replace(LegionMemoryPool* p, int32_t replace) { return pool_set_mode_field(p, &SampleMode::replace, replace); }
extern "C" int32_t legion_pool_sample_replace(const LegionMemoryPool* p) { return pool_mode_field(p, &SampleMode::replace); }
extern "C" int32_t legion_pool_set_edge_ids(LegionMemoryPool* p, int32_t on) { return pool_set_mode_field(p, &SampleMode::edge_ids, on); }
extern "C" int32_t legion_pool_edge_ids(const LegionMemoryPool* p) { return pool_mode_field(p, &SampleMode::edge_ids); }
extern "C" int32_t legion_pool_set_sample_weighted(LegionMemoryPool* p, int32_t on) { return pool_set_mode_field(p, &SampleMode::weighted, on); }
extern "C" int32_t legion_pool_sample_weighted(const LegionMemoryPool* p) { return pool_mode_field(p, &SampleMode::weighted); }

extern "C" void legion_pool_set_current_pipe(LegionMemoryPool* p_, int32_t pipe)
{
    MemoryPool* mp = reinterpret_cast<MemoryPool*>(p_);
    if (mp) mp->SetCurrentPipe(pipe % mp->PipelineDepth());
}

extern "C" void legion_pool_set_mode_iter(LegionMemoryPool* p_, int32_t mode, int32_t iter)
{
    MemoryPool* mp = reinterpret_cast<MemoryPool*>(p_);
    if (mp) { mp->SetCurrentMode(mode); mp->SetIter(iter); }
}

extern "C" int32_t legion_pool_num_ids(const LegionMemoryPool* p_)
{
    const MemoryPool* mp = reinterpret_cast<const MemoryPool*>(p_);
    return mp ? mp->num_ids : 0;
}

extern "C" void* legion_pool_buffer(LegionMemoryPool* p_, int32_t which)
{
    MemoryPool* mp = reinterpret_cast<MemoryPool*>(p_);
    if (!mp) return nullptr;
    switch (which) {
        case 0: return mp->GetSampledIds();
        case 1: return mp->GetFloatFeatures();
        case 2: return mp->GetLabels();
        case 3: return mp->GetAggSrcOf();
        case 4: return mp->GetAggDstOf();
        case 5: return mp->GetNodeCounter();
        case 6: return mp->GetEdgeCounter();
        case 7: return mp->GetAggSrcId();
        case 8: return mp->GetAggDstId();
        case 9: return mp->GetCacheSearchBuffer();
        case 10: return mp->GetTmpPartIdx();
        case 11: return mp->GetTmpPartOff();
        case 12: return mp->GetPositionMap();      // always null: no per-vertex state in this build
        case 13: return mp->node_slot;             // [num_ids] feature-cache slot carried per node (LG_FS_UNKNOWN = -3: look it up), or null
        case 14: return mp->mode.edge_ids ? mp->agg_edge_ids : nullptr;      // int64[num_ids], edge-id mode only (legion_pool_set_edge_ids)
        default: return nullptr;
    }
}

// LG_ERR_* bits raised by the kernels for this pool since it was created (0 = none); host-visible memory,
// valid once the batch has completed
extern "C" int32_t legion_pool_error(const LegionMemoryPool* p_)
{
    const MemoryPool* mp = reinterpret_cast<const MemoryPool*>(p_);
    return mp ? mp->ErrorBits() : 0;
}

// hash buckets per lane of the first-touch de-duplication: 8, 16, 64 or 256
extern "C" int32_t legion_pool_lds_buckets(const LegionMemoryPool* p_)
{
    const MemoryPool* p = reinterpret_cast<const MemoryPool*>(p_);
    return p ? (1 << p->lds_bucket_bits) : 0;
}

extern "C" int64_t legion_pool_state_bytes(const LegionMemoryPool* p_)
{
    const MemoryPool* mp = reinterpret_cast<const MemoryPool*>(p_);
    if (!mp) return 0;
    // one hop's claim lists + the known lists (nothing that scales with the graph), as the pool's plan sized them
    return mp->private_plan.bytes_of(PA_CLAIM_PAIRS) + mp->private_plan.bytes_of(PA_KNOWN_PAIRS);
}

extern "C" void legion_pool_destroy(LegionMemoryPool* p_)
{
    MemoryPool* mp = reinterpret_cast<MemoryPool*>(p_);
    if (!mp) return;
    mp->Finalize();
    delete mp;
}
