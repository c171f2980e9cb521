// vmm_map.h -- another process's device memory, received as file descriptors of its physical chunks and mapped back to back.  The one
// routine behind both receivers: the trainer end mapping the server's lane arena (ipc_service.cpp) and a clique member mapping
// another member's (storage.hip lg_scattered_map_remote).  Header-only like vmm_probe.h and for the same reason: each of the two
// runs on its own HIP runtime.  The sending side is storage.hip lg_scattered_serve; the messages are ipc_wire.h's.
#pragma once
#include "../csrc/ipc_wire.h"
#include "vmm_probe.h"      // vmm_import_fd(): imports a received descriptor whichever way THIS process's HIP runtime takes one

// gives back the first n_mapped chunks of a range of n_chunks x chunk_bytes at `base`, and the range
static void vmm_unmap_chunks(void* base, int n_mapped, int n_chunks, long long chunk_bytes)
{
    if (base == nullptr) return;
    for (int i = 0; i < n_mapped; i++)
        if (hipMemUnmap((char*)base + (size_t)i * (size_t)chunk_bytes, (size_t)chunk_bytes) != hipSuccess) (void)hipGetLastError();
    if (hipMemAddressFree(base, (size_t)n_chunks * (size_t)chunk_bytes) != hipSuccess) (void)hipGetLastError();
}

// Connect to the abstract socket `socket_name` (a same-user peer only), receive n_chunks descriptors, import and map them in order,
// accessible to hip_dev.  A descriptor is closed and its import handle released as soon as its chunk is mapped (the mapping keeps the
// memory alive, nothing else has to): an arena has thousands of chunks, a process a limit on open descriptors.  On any failure what
// was mapped is unmapped again, the range given back and null returned, with the failed step in *why.
static void* vmm_map_chunks(const char* socket_name, int n_chunks, long long chunk_bytes, int hip_dev, const char** why)
{
    const int c = wire_connect_same_user(socket_name, why);
    if (c < 0) return nullptr;
    const size_t bytes = (size_t)n_chunks * (size_t)chunk_bytes;
    void* base = nullptr;
    if (hipMemAddressReserve(&base, bytes, 0, nullptr, 0) != hipSuccess) { (void)hipGetLastError(); close(c); *why = "hipMemAddressReserve"; return nullptr; }
    int got = 0;
    bool ok = true;
    while (got < n_chunks && ok) {
        int fds[WIRE_FD_BATCH];
        const int n = wire_recv_fd_batch(c, fds);
        if (n < 0) { *why = "recvmsg()"; ok = false; break; }
        for (int i = 0; i < n; i++) {
            if (ok && got < n_chunks) {
                hipMemGenericAllocationHandle_t h;
                if (vmm_import_fd(&h, fds[i]) != hipSuccess) { (void)hipGetLastError(); *why = "hipMemImportFromShareableHandle"; ok = false; }
                else {
                    if (hipMemMap((char*)base + (size_t)got * (size_t)chunk_bytes, (size_t)chunk_bytes, 0, h, 0) != hipSuccess) { (void)hipGetLastError(); *why = "hipMemMap"; ok = false; }
                    else got++;
                    if (hipMemRelease(h) != hipSuccess) (void)hipGetLastError();      // (mapped or not: the handle is not needed again)
                }
            }
            close(fds[i]);
        }
    }
    close(c);
    if (ok) {
        hipMemAccessDesc acc = {};
        acc.location.type = hipMemLocationTypeDevice;
        acc.location.id = hip_dev;
        acc.flags = hipMemAccessFlagsProtReadWrite;
        if (hipMemSetAccess(base, bytes, &acc, 1) != hipSuccess) { (void)hipGetLastError(); *why = "hipMemSetAccess"; ok = false; }
    }
    if (!ok) {
        vmm_unmap_chunks(base, got, n_chunks, chunk_bytes);
        return nullptr;
    }
    return base;
}
