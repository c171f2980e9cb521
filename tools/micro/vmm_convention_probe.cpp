// Prints how the HIP runtime this program is linked against takes a file-descriptor handle in hipMemImportFromShareableHandle:
//   hipcc -O2 tools/micro/vmm_convention_probe.cpp -o /tmp/vmm_convention_probe && /tmp/vmm_convention_probe
// -> "convention <0 pointer | 1 value | -1 none> runtime <hipRuntimeGetVersion>".  The trainer end (legion_amd/trainer/ipc_service.cpp)
// runs the same probe on the runtime bundled with torch: ipc_service.vmm_fd_convention().
//
//   vmm_convention_probe --map <abstract socket> <chunks> <chunk bytes> <device>
// maps the chunks another process serves on that socket (storage.hip lg_scattered_serve) and gives them back: exit status 0 when
// that worked, 1 with the failed step otherwise.  The library starts it once to find out whether device memory can cross a process
// boundary as file descriptors on this machine at all (storage.hip lg_fd_handover_works).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../legion_amd/trainer/vmm_map.h"

int main(int argc, char** argv)
{
    if (argc == 6 && strcmp(argv[1], "--map") == 0) {
        const int n_chunks = atoi(argv[3]), dev = atoi(argv[5]);
        const long long chunk_bytes = atoll(argv[4]);
        if (n_chunks < 1 || chunk_bytes < 1 || hipSetDevice(dev) != hipSuccess) { printf("no device\n"); return 2; }
        const char* why = "";
        void* base = vmm_map_chunks(argv[2], n_chunks, chunk_bytes, dev, &why);
        if (base == nullptr) { printf("not mapped (%s)\n", why); return 1; }
        vmm_unmap_chunks(base, n_chunks, n_chunks, chunk_bytes);
        printf("mapped\n");
        return 0;
    }
    int v = 0;
    (void)hipRuntimeGetVersion(&v);
    if (hipSetDevice(0) != hipSuccess) { printf("no device\n"); return 2; }
    printf("convention %d runtime %d\n", vmm_fd_convention(), v);
    return 0;
}
