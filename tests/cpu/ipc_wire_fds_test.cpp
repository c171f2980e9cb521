// The descriptor passing of legion_amd/csrc/ipc_wire.h end to end inside one process, built with AddressSanitizer +
// UndefinedBehaviorSanitizer (oracle/Makefile, target san): a thread listens on an abstract socket and sends the descriptors of n
// temporary files in messages of at most WIRE_FD_BATCH through wire_send_fd_batch; the main thread takes them through
// wire_connect_same_user and wire_recv_fd_batch, message by message, and compares the files' inode numbers in order.  n = 1, 64, 65
// and 130: one descriptor, one full message, the first split, three messages with a short last one.  Then a sender that closes
// after one message of two: the receiver must get -1, not wait and not invent descriptors.
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include <sys/stat.h>

#include "../../legion_amd/csrc/ipc_wire.h"

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("MISMATCH "); printf(__VA_ARGS__); printf("\n"); g_bad++; } } while (0)

static ino_t inode_of(int fd)
{
    struct stat st;
    return fstat(fd, &st) == 0 ? st.st_ino : 0;
}

// sends `send` of the files' descriptors to the first peer, then closes the connection
static void serve(int ls, const std::vector<int>& files, int send)
{
    const int c = accept4(ls, nullptr, nullptr, SOCK_CLOEXEC);
    if (c < 0) return;
    for (int i0 = 0; i0 < send; i0 += WIRE_FD_BATCH) {
        const int n = send - i0 < WIRE_FD_BATCH ? send - i0 : WIRE_FD_BATCH;
        if (wire_send_fd_batch(c, files.data() + i0, n) != 0) break;
    }
    close(c);
}

// n files, of which the sender hands over `send` before it closes
static void one_round(int n, int send, int round)
{
    char name[WIRE_NAME_MAX];
    wire_bulk_socket_name(name, sizeof(name), (int)getpid(), round);
    std::vector<int> files;
    std::vector<ino_t> inodes;
    for (int i = 0; i < n; i++) {
        FILE* f = tmpfile();
        if (f == nullptr) { printf("MISMATCH tmpfile()\n"); g_bad++; return; }
        files.push_back(dup(fileno(f)));
        fclose(f);
        inodes.push_back(inode_of(files.back()));
    }
    const int ls = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
    sockaddr_un addr;
    const socklen_t len = wire_abstract_address(&addr, name);
    CHECK(ls >= 0 && bind(ls, (sockaddr*)&addr, len) == 0 && listen(ls, 4) == 0, "n %d: no listening socket", n);
    std::thread sender(serve, ls, std::cref(files), send);

    const char* why = "";
    const int c = wire_connect_same_user(name, &why);
    CHECK(c >= 0, "n %d: wire_connect_same_user failed at %s", n, why);
    int got = 0, messages = 0, last = 0, ended = 0;
    while (c >= 0 && got < n) {
        int fds[WIRE_FD_BATCH];
        const int k = wire_recv_fd_batch(c, fds);
        if (k < 0) { ended = k; break; }
        messages++;
        last = k;
        for (int i = 0; i < k; i++) {
            if (got < n) {
                CHECK(fds[i] != files[(size_t)got] && inode_of(fds[i]) == inodes[(size_t)got], "n %d: descriptor %d is not file %d", n, got, got);
                got++;
            }
            close(fds[i]);      // as soon as it has been looked at: never more than one message's worth open
        }
    }
    if (c >= 0) close(c);
    sender.join();
    close(ls);
    for (int fd : files) close(fd);
    if (send == n) {
        CHECK(got == n, "n %d: %d descriptors arrived", n, got);
        CHECK(messages == (n + WIRE_FD_BATCH - 1) / WIRE_FD_BATCH, "n %d: %d messages", n, messages);
        CHECK(last == (n - 1) % WIRE_FD_BATCH + 1, "n %d: the last message held %d", n, last);
    } else {
        CHECK(got == send && ended == -1, "n %d, peer closed after %d: %d descriptors arrived, then %d", n, send, got, ended);
    }
}

int main()
{
    int round = 0;
    for (int n : {1, 64, 65, 130}) one_round(n, n, round++);
    one_round(5, 2, round++);          // the peer closes early: -1 after the one message it sent
    {   // nobody listens: the failed step, and no descriptor left behind
        const char* why = "";
        const int c = wire_connect_same_user("legion_bulk_0_no_such_socket", &why);
        CHECK(c == -1 && why[0] == 'c', "a connection to nobody: %d (%s)", c, why);
    }
    {   // a batch is 1 .. WIRE_FD_BATCH descriptors
        int fds[WIRE_FD_BATCH + 1] = {0};
        CHECK(wire_send_fd_batch(-1, fds, 0) == -1 && wire_send_fd_batch(-1, fds, WIRE_FD_BATCH + 1) == -1, "a batch of 0 or 65 was not refused");
    }
    printf("%d rounds, %d failed\n", round, g_bad);
    return g_bad ? 1 : 0;
}
