// Pins the server <-> trainer wire format (legion_amd/csrc/ipc_wire.h) over a literal table: the size of the two shared-memory
// layouts and the offset of every field, the magic, the version and its thresholds, the slots of the slab's handles, the counter
// indices and every name.  The numbers were computed on the CPU from the structs of the commit before the header existed (three hand
// copies then), not from the header: a trainer built then must read the same bytes from a server built now.
//   g++ -O1 -std=c++17 -I include ipc_wire_test.cpp -o t && ./t
#include <cstdio>
#include <cstring>

#include "../../legion_amd/csrc/ipc_wire.h"

struct Number { const char* what; long long got, want; };
static const Number numbers[] = {
    {"sizeof(shmStruct)", sizeof(shmStruct), 7180},
    {"memHandle", offsetof(shmStruct, memHandle), 12},
    {"sizeof(shmExt)", sizeof(shmExt), 3544},
    {"ext_magic", offsetof(shmExt, ext_magic), 0},
    {"ext_version", offsetof(shmExt, ext_version), 4},
    {"server_state", offsetof(shmExt, server_state), 8},
    {"counters", offsetof(shmExt, counters), 16},
    {"arena", offsetof(shmExt, arena), 2064},
    {"arena_bytes", offsetof(shmExt, arena_bytes), 2576},
    {"trainer_direct", offsetof(shmExt, trainer_direct), 2640},
    {"view_on", offsetof(shmExt, view_on), 2672},
    {"view", offsetof(shmExt, view), 2736},
    {"arena_kind", offsetof(shmExt, arena_kind), 3376},
    {"arena_chunks", offsetof(shmExt, arena_chunks), 3408},
    {"arena_chunk_bytes", offsetof(shmExt, arena_chunk_bytes), 3440},
    {"arena_sock_pid", offsetof(shmExt, arena_sock_pid), 3504},
    {"feature_out_dtype", offsetof(shmExt, feature_out_dtype), 3512},
    {"sizeof(wireIpcHandle)", sizeof(wireIpcHandle), 64},

    {"the magic", LEGION_SHM_EXT_MAGIC, 0x4C47494F},
    {"the version", LEGION_SHM_EXT_VERSION, 4},
    {"views since", LEGION_SHM_EXT_HAS_VIEWS, 2},
    {"chunked arenas since", LEGION_SHM_EXT_HAS_CHUNKED_ARENA, 3},
    {"the feature dtype since", LEGION_SHM_EXT_HAS_FEATURE_DTYPE, 4},

    {"slot ids", WIRE_SLOT_IDS, 0},
    {"slot features", WIRE_SLOT_FEATURES, 1},
    {"slot labels", WIRE_SLOT_LABELS, 2},
    {"slot agg_src", WIRE_SLOT_AGG_SRC, 3},
    {"slot agg_dst", WIRE_SLOT_AGG_DST, 4},
    {"slot node_counter", WIRE_SLOT_NODE_COUNTER, 5},
    {"slot edge_counter", WIRE_SLOT_EDGE_COUNTER, 6},

    {"rows of a batch, 1 hop", wire_rows_index(1), 10},
    {"rows of a batch, 2 hops", wire_rows_index(2), 11},
    {"rows of a batch, 6 hops", wire_rows_index(6), 15},
    {"edges of a batch, 1 hop", wire_edges_index(1), 26},
    {"edges of a batch, 2 hops", wire_edges_index(2), 27},
    {"edges of a batch, 6 hops", wire_edges_index(6), 31},
    {"the edge counters", WIRE_EDGE_COUNTERS, 16},
    {"descriptors per message", WIRE_FD_BATCH, 64},
};

int main()
{
    int bad = 0, n = 0;
    for (const Number& c : numbers) {
        n++;
        if (c.got != c.want) { printf("MISMATCH %s: got %lld, want %lld\n", c.what, c.got, c.want); bad++; }
    }
    char buf[WIRE_NAME_MAX];
    // each builder at one input; the returned length is snprintf's
    auto take = [&](const char* what, int len, const char* want) {
        n++;
        if (strcmp(buf, want) != 0 || len != (int)strlen(want)) { printf("MISMATCH %s: got \"%s\" (%d), want \"%s\"\n", what, buf, len, want); bad++; }
    };
    take("the slab", wire_slab_name(buf, sizeof(buf), "_ns"), "simpleIPCshm_ns");
    take("the mirror object", wire_mirror_name(buf, sizeof(buf), ""), "legionIPCext");
    take("the free semaphore", wire_sem_r_name(buf, sizeof(buf), 0, 1, ""), "sem_r_0_1");
    take("the ready semaphore", wire_sem_w_name(buf, sizeof(buf), 3, 1, "_ns"), "sem_w_3_1_ns");
    take("the arena socket", wire_arena_socket_name(buf, sizeof(buf), 4711, 7), "legion_arena_4711_7");
    take("the bulk socket", wire_bulk_socket_name(buf, sizeof(buf), 4711, 12), "legion_bulk_4711_12");
    // an abstract address: a leading zero byte, then the name, and nothing after it counts
    sockaddr_un addr;
    const socklen_t len = wire_abstract_address(&addr, "legion_arena_1_0");
    n++;
    if (addr.sun_family != AF_UNIX || addr.sun_path[0] != 0 || strcmp(addr.sun_path + 1, "legion_arena_1_0") != 0 ||
        len != (socklen_t)(offsetof(sockaddr_un, sun_path) + 1 + 16)) {
        printf("MISMATCH the abstract address: length %d\n", (int)len);
        bad++;
    }
    printf("%d cases, %d failed\n", n, bad);
    return bad ? 1 : 0;
}
