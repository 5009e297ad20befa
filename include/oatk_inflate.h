/*
 * include/oatk_inflate.h -- the member table of a BGZF file, for oatk_hip_inflate_bgzf (include/oatk_hip_ingest.h).  Host code, in liboatk_host.
 */
#ifndef OATK_INFLATE_H
#define OATK_INFLATE_H

#include "oatk_hip_ingest.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Walk n_bytes of a BGZF file header by header, from buf[0], and list the members found -- nothing is inflated: a member says how long it is (its BC field) and how
 * much text it holds (ISIZE).  The walk ends at the first of: the end of the bytes, bytes that are no whole BGZF member (a plain gzip member, a cut one), a member
 * whose text would take the total past text_cap, member_cap members.  These are the members the host reader (host/gzsrc.c) would inflate in one go into a buffer of
 * text_cap bytes -- the two share the code that reads a member's header.  in_off is relative to buf, out_off to the start of the text; *comp_bytes = the compressed
 * bytes the listed members cover (the next member, if any, begins there), *text_bytes = their text. */
int oatk_bgzf_index(const uint8_t *buf, uint64_t n_bytes, uint64_t text_cap, uint64_t member_cap, oatk_bgzf_member_t *members, uint64_t *n_members,
                    uint64_t *text_bytes, uint64_t *comp_bytes);

/* The streamed reader (oatk_sr_read_files and what is built on it) inflates the BGZF members of its input ON THE DEVICE when this is on: the compressed bytes are
 * staged and uploaded, oatk_hip_inflate_bgzf writes the text into the window, read names are cut there (oatk_hip_ingest_names).  A window with a member the device
 * refuses is inflated again by the host path, which alone decides whether the file is damaged: the switch never changes which files are read or what is read from
 * them.  Plain gzip members, pipes and members cut by a window's end stay on the host.  Off by default; the environment variable OATK_DEVICE_INFLATE=1, read once,
 * turns it on for callers that cannot call this (the CLI). */
void oatk_host_set_device_inflate(int on);
/* since the process began: members inflated on the device, members inflated again on the host after the device refused one, windows that hold device-inflated text */
void oatk_host_inflate_counts(uint64_t out[3]);

#ifdef __cplusplus
}
#endif
#endif
