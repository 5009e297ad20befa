// oatk_amd/csrc/ingest_names.hpp -- read names cut out of text that lies on the device (oatk_hip_ingest_names): a window whose text was inflated on the device has no
// copy on the host to cut them from.  A name is what follows the header character up to the first space, tab, CR or LF, or the end of the text (kseq.h: ks_getuntil
// with KS_SEP_SPACE; host/ingest_host.c: hname_worker reads the same from the host's copy).
#pragma once
#include "common.hpp"

namespace oatk {

// len[i] = length of the name of record i (len[n] = 0: the scan's sentinel)
__global__ __launch_bounds__(256) void ing_name_len_kernel(const uint8_t *__restrict__ text, uint64_t n_bytes, const uint64_t *__restrict__ hdr, uint64_t n, uint64_t *__restrict__ len)
{
    const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    uint64_t l = 0;
    if (i < n) {
        const uint64_t p = hdr[i] + 1;                  // behind '>' / '@'
        uint64_t e = p;
        while (e < n_bytes) { const uint8_t c = text[e]; if (c == ' ' || c == '\t' || c == '\n' || c == '\r') break; ++e; }
        l = e > p? e - p : 0;                           // (a header character that ends the text has an empty name)
    }
    len[i] = l;
}

// out = off[0 .. n] followed by the names back to back: what one copy takes to the host
__global__ __launch_bounds__(256) void ing_name_copy_kernel(const uint8_t *__restrict__ text, const uint64_t *__restrict__ hdr, uint64_t n, const uint64_t *__restrict__ off, uint8_t *__restrict__ out)
{
    const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    uint64_t *out_off = (uint64_t *) out;
    uint8_t *packed = out + (n + 1) * 8;
    const uint64_t o = off[i];
    out_off[i] = o;
    if (i == n) return;
    const uint64_t l = off[i + 1] - o, p = hdr[i] + 1;
    for (uint64_t k = 0; k < l; ++k) packed[o + k] = text[p + k];
}

}  // namespace oatk
