/* ipc_wire.h -- the server <-> trainer wire format, once: the two shared-memory layouts, the names of every object the two ends
 * meet at, the counter block, and the passing of file descriptors between processes.  Host only, C11 and C++17, no HIP: the server
 * end (ipc_env.hip, storage.hip, pipeline.hip, server.hip: hipcc against /opt/rocm), the trainer end (trainer/ipc_service.cpp: the HIP
 * runtime bundled with torch) and the protocol-only consumer (tools/boundary_consumer.c: plain C) include this file and nothing else
 * says what the boundary looks like.  tests/cpu/ipc_wire_test.cpp pins every offset, number and name below over a literal table; a
 * new protocol version changes this header and that table.
 *
 * Reference: SS/engine/ipc_service.cu:28-31 and TB/ipc_cuda_kernel.cu:30-33 (the slab), SS/engine/ipc_service.cu:181-192 (names).
 * In C, include this file before any system header: struct ucred (SO_PEERCRED) needs _GNU_SOURCE. */
#ifndef LEGION_IPC_WIRE_H
#define LEGION_IPC_WIRE_H
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include <assert.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/socket.h>
#include <sys/un.h>
#include <unistd.h>

#include "../../include/legion_hip.h"

/* the reference's spellings of the sizing constants (SS/include/system_config.cuh:47-57), which code ported from it uses */
#define INTERBATCH_CON LEGION_INTERBATCH_CON
#define INTRABATCH_CON LEGION_INTRABATCH_CON
#define MAX_DEVICE LEGION_MAX_DEVICE
#define MEMORY_USAGE LEGION_MEMORY_USAGE

/* An IPC memory handle (hipIpcMemHandle_t, like cudaIpcMemHandle_t): 64 opaque bytes.  A translation unit that sees HIP asserts
 * sizeof(hipIpcMemHandle_t) == 64 and casts. */
typedef struct wireIpcHandle_st { char reserved[64]; } wireIpcHandle;

/* memHandle[dev][pipe][k]: the seven buffers of a pipe slot */
enum { WIRE_SLOT_IDS = 0, WIRE_SLOT_FEATURES = 1, WIRE_SLOT_LABELS = 2, WIRE_SLOT_AGG_SRC = 3, WIRE_SLOT_AGG_DST = 4,
       WIRE_SLOT_NODE_COUNTER = 5, WIRE_SLOT_EDGE_COUNTER = 6 };

/* The slab is the reference's, byte for byte and no larger: a trainer built from the reference opens it with shm_open +
 * ftruncate(sizeof(its struct)) (TB/helper_multiprocess.cpp:30-37), which must not change its size. */
typedef struct shmStruct_st {
    int32_t steps[3];                                                                       /* train, valid, test */
    wireIpcHandle memHandle[LEGION_MAX_DEVICE][LEGION_INTERBATCH_CON][LEGION_MEMORY_USAGE];
} shmStruct;
static_assert(offsetof(shmStruct, memHandle) == 12 &&
              sizeof(shmStruct) == 12 + LEGION_MAX_DEVICE * LEGION_INTERBATCH_CON * LEGION_MEMORY_USAGE * 64,
              "the reference's slab layout is the wire format");

/* This build's extra lives in a shm object of its own, the mirror: registered with HIP and written by the GPU on the server side,
 * opened by this build's trainer end when it exists (never created there) and believed when its magic says so.
 *   version 1: per (device, pipe slot) the 16 + 16 counters of the batch in that slot in HOST memory, so the trainer end needs no
 *     device-to-host copy per batch (the reference does two blocking 64-byte cudaMemcpy per get_next, TB/ipc_cuda_kernel.cu:186-187).
 *   version 2, the "direct view" hand-over: the server produces mini-batches in launch groups into per-lane buffers (server.hip) that
 *     all live in ONE device allocation per GPU, the lane arena; its IPC handle is published here.  A trainer end that can open it says
 *     so in trainer_direct[dev] BEFORE its first sem_post; from then on a hand-over is no GPU work at all: the server writes, per
 *     (device, pipe slot), where the five trainer-visible arrays of the batch start inside the arena and posts sem_w -- same semaphores,
 *     same two-slot order, and the slab above stays valid for a trainer that knows nothing of this (it gets copies in the slot buffers;
 *     LEGION_NO_DIRECT_VIEWS=1 keeps this build's trainer end on them too).
 *   version 3: the arena may be built from physical chunks mapped in shuffled order (storage.hip d_alloc_scattered: the gathers then
 *     write a group's rows all over the HBM, +7 %), which hipIpcGetMemHandle cannot export.  arena_kind 1: `arena` is unused; the
 *     trainer connects to the abstract unix socket wire_arena_socket_name(arena_sock_pid, dev), receives arena_chunks file descriptors
 *     (SCM_RIGHTS, in mapping order), imports each and maps them back to back: arena_chunks x arena_chunk_bytes >= arena_bytes.
 *   version 4: the dtype of the feature rows of each server GPU's batches (LEGION_FEATURE_*; 1 = bf16[n x D]), in the pipe slots and in
 *     the views alike.  A trainer end that reads an older version takes float32 rows. */
#define LEGION_SHM_EXT_MAGIC 0x4C47494F   /* "LGIO" */
#define LEGION_SHM_EXT_VERSION 4
#define LEGION_SHM_EXT_HAS_VIEWS 2            /* ext_version >= this: the fields from `arena` to `view` exist */
#define LEGION_SHM_EXT_HAS_CHUNKED_ARENA 3    /* ... those from `arena_kind` to `arena_sock_pid` */
#define LEGION_SHM_EXT_HAS_FEATURE_DTYPE 4    /* ... feature_out_dtype */
typedef struct shmExt_st {
    int32_t ext_magic;                                                        /* LEGION_SHM_EXT_MAGIC once the fields below are live */
    int32_t ext_version;
    int32_t server_state;                                                     /* 0 serving, 1 the server stopped on an error (trainers must not wait) */
    int32_t ext_reserved;
    int32_t counters[LEGION_MAX_DEVICE][LEGION_INTERBATCH_CON][32];           /* [0..15] node_counter, [16..31] edge_counter */
    wireIpcHandle arena[LEGION_MAX_DEVICE];                                   /* lane arena of each server GPU, valid when arena_bytes > 0 */
    int64_t arena_bytes[LEGION_MAX_DEVICE];
    int32_t trainer_direct[LEGION_MAX_DEVICE];                                /* written by the trainer end: 1 = it opened the arena and takes views */
    int32_t view_on[LEGION_MAX_DEVICE][LEGION_INTERBATCH_CON];                /* 1: the batch in this slot is the view below, 0: it is in the slot's buffers */
    int64_t view[LEGION_MAX_DEVICE][LEGION_INTERBATCH_CON][5];                /* byte offsets into the arena: ids, features, labels, agg_src, agg_dst */
    int32_t arena_kind[LEGION_MAX_DEVICE];
    int32_t arena_chunks[LEGION_MAX_DEVICE];
    int64_t arena_chunk_bytes[LEGION_MAX_DEVICE];
    int32_t arena_sock_pid;
    int32_t ext_reserved2;
    int32_t feature_out_dtype[LEGION_MAX_DEVICE];
} shmExt;

/* ---- the counter block of a batch: 16 node counters, then 16 edge counters.  Word INTRABATCH_CON * 3 + h of either half is the
 *      cumulative count after hop h (SS/engine/operator_impl.cu), so the batch's rows and edges are the words at its hop count ---- */
#define WIRE_EDGE_COUNTERS 16             /* where the edge counters start in counters[dev][pipe][] */
static inline int wire_rows_index(int hops) { return LEGION_INTRABATCH_CON * 3 + hops; }
static inline int wire_edges_index(int hops) { return WIRE_EDGE_COUNTERS + LEGION_INTRABATCH_CON * 3 + hops; }

/* ---- names: snprintf into the caller's buffer (WIRE_NAME_MAX holds any of them with a namespace suffix up to NAME_MAX).  `sfx` is
 *      LEGION_IPC_NAMESPACE or "": it lets independent servers (tests) share a host. ---- */
#define WIRE_NAME_MAX 320
static inline int wire_slab_name(char* buf, size_t n, const char* sfx) { return snprintf(buf, n, "simpleIPCshm%s", sfx); }
static inline int wire_mirror_name(char* buf, size_t n, const char* sfx) { return snprintf(buf, n, "legionIPCext%s", sfx); }
/* sem_r, trainer -> server: the buffers of (dev, pipe) are free; sem_w, server -> trainer: a batch is ready in them */
static inline int wire_sem_r_name(char* buf, size_t n, int dev, int pipe, const char* sfx) { return snprintf(buf, n, "sem_r_%d_%d%s", dev, pipe, sfx); }
static inline int wire_sem_w_name(char* buf, size_t n, int dev, int pipe, const char* sfx) { return snprintf(buf, n, "sem_w_%d_%d%s", dev, pipe, sfx); }
/* abstract unix sockets that hand out the chunks of a server GPU's lane arena / of a clique member's (peer_gather = bulk) */
static inline int wire_arena_socket_name(char* buf, size_t n, int pid, int dev) { return snprintf(buf, n, "legion_arena_%d_%d", pid, dev); }
static inline int wire_bulk_socket_name(char* buf, size_t n, int pid, int tag) { return snprintf(buf, n, "legion_bulk_%d_%d", pid, tag); }

/* ---- file descriptors between processes: SCM_RIGHTS messages of one payload byte and at most WIRE_FD_BATCH descriptors ---- */
#define WIRE_FD_BATCH 64
typedef union wireFdControl_un {
    struct cmsghdr align;
    char buf[CMSG_SPACE(sizeof(int) * WIRE_FD_BATCH)];
} wireFdControl;

/* the address of the abstract socket `name`; returns its length for bind() / connect() */
static inline socklen_t wire_abstract_address(struct sockaddr_un* addr, const char* name)
{
    memset(addr, 0, sizeof(*addr));
    addr->sun_family = AF_UNIX;
    const int len = snprintf(addr->sun_path + 1, sizeof(addr->sun_path) - 1, "%s", name);
    return (socklen_t)(offsetof(struct sockaddr_un, sun_path) + 1 + (size_t)len);
}

/* A connected socket to the abstract unix socket `name`, or -1 with the failed step in *why.  Whoever answers under that name hands
 * out descriptors this process will map: it must be a process of the same user (the abstract namespace has no file permissions). */
static inline int wire_connect_same_user(const char* name, const char** why)
{
    const int c = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
    if (c < 0) { *why = "socket()"; return -1; }
    struct sockaddr_un addr;
    const socklen_t len = wire_abstract_address(&addr, name);
    if (connect(c, (struct sockaddr*)&addr, len) != 0) { close(c); *why = "connect()"; return -1; }
    struct ucred cr;
    socklen_t cl = sizeof(cr);
    if (getsockopt(c, SOL_SOCKET, SO_PEERCRED, &cr, &cl) != 0 || cr.uid != geteuid()) { close(c); *why = "the socket belongs to another user"; return -1; }
    return c;
}

/* one message with fds[0..n), 1 <= n <= WIRE_FD_BATCH; 0 when it went out.  The descriptors stay the caller's. */
static inline int wire_send_fd_batch(int sock, const int* fds, int n)
{
    if (n < 1 || n > WIRE_FD_BATCH) return -1;
    char payload = 'f';
    struct iovec io = {&payload, 1};
    wireFdControl ctl;
    memset(&ctl, 0, sizeof(ctl));
    struct msghdr msg;
    memset(&msg, 0, sizeof(msg));
    msg.msg_iov = &io; msg.msg_iovlen = 1; msg.msg_control = ctl.buf; msg.msg_controllen = CMSG_SPACE(sizeof(int) * (size_t)n);
    struct cmsghdr* cm = CMSG_FIRSTHDR(&msg);
    cm->cmsg_level = SOL_SOCKET; cm->cmsg_type = SCM_RIGHTS; cm->cmsg_len = CMSG_LEN(sizeof(int) * (size_t)n);
    memcpy(CMSG_DATA(cm), fds, sizeof(int) * (size_t)n);
    return sendmsg(sock, &msg, MSG_NOSIGNAL) == 1 ? 0 : -1;
}

/* one message: its descriptors into fds[WIRE_FD_BATCH] (close-on-exec; the caller closes them); how many arrived, or -1 (the peer
 * closed, an error, or a message without descriptors) */
static inline int wire_recv_fd_batch(int sock, int* fds)
{
    char payload = 0;
    struct iovec io = {&payload, 1};
    wireFdControl ctl;
    struct msghdr msg;
    memset(&msg, 0, sizeof(msg));
    msg.msg_iov = &io; msg.msg_iovlen = 1; msg.msg_control = ctl.buf; msg.msg_controllen = sizeof(ctl.buf);
    if (recvmsg(sock, &msg, MSG_CMSG_CLOEXEC) != 1) return -1;
    struct cmsghdr* cm = CMSG_FIRSTHDR(&msg);
    if (cm == NULL || cm->cmsg_level != SOL_SOCKET || cm->cmsg_type != SCM_RIGHTS) return -1;
    const int n = (int)((cm->cmsg_len - CMSG_LEN(0)) / sizeof(int));
    memcpy(fds, CMSG_DATA(cm), sizeof(int) * (size_t)n);
    return n;
}

#endif
