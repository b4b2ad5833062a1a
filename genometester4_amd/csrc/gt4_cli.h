/* gt4_cli.h -- what the three drop-in command lines (glistcompare, glistquery, glistmaker) repeat, once.  gt4_cli.c is
 * compiled into each executable and is no part of libgt4hip.so.  The argv loops, option enums, help texts and the
 * reference's own messages stay with each tool. */
#ifndef GT4_CLI_H
#define GT4_CLI_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "gt4hip.h"

#define DOWNLOAD_CHUNK (4u << 20) /* records per device -> host -> file step (48 MiB) */
#define CHK(ctx, call)                                                            \
  do {                                                                            \
    if ((call) != GT4HIP_OK) {                                                    \
      fprintf (stderr, "Error: %s: %s\n", #call, gt4hip_last_error (ctx));        \
      exit (1);                                                                   \
    }                                                                             \
  } while (0)

typedef struct { const char *name; int opt; } GT4CliOption;

/* the `opt` of the entry named `arg`, or -1 */
int gt4_cli_find_option (const GT4CliOption *options, size_t n_options, const char *arg);
/* "<tool> version <major>.<minor>.<micro> (<qualifier>)"; the help is that line, then `lines` */
void gt4_cli_print_version (FILE *to, const char *tool);
void gt4_cli_print_help (FILE *to, const char *tool, const char *const *lines, size_t n_lines);
/* "<n>[K|M|G]" -> bytes; 0 for NULL, "" and anything not positive */
uint64_t gt4_cli_parse_bytes (const char *s);
/* GT4HIP_DEVICE=N (default 0) and GT4HIP_VERBOSE=1 */
void gt4_cli_read_environment (int *device, int *verbose);
/* 1 after the refusal message if c0, c1 (the first two bytes of `name`; EOF where there is none) are the gzip magic */
int gt4_cli_refuse_gzip (const char *name, int c0, int c1);

/* bytes of the sequence name that starts at `name_pos` of the `size` bytes of a FastA / FastQ file: up to the first byte
 * <= ' ' or the end of the file; 0 where name_pos lies behind the file */
uint64_t gt4_cli_name_length (const unsigned char *data, uint64_t size, uint64_t name_pos);

/* glistquery --mask writes a stream, and a hit word of the next piece may still cover the end of what has been masked so
 * far: the tail from the (k - 1)-th last byte >= ' ' on is held back.  push: the last `back` bytes >= ' ' of the held tail are
 * replaced (by mask_byte, soft: by byte | 0x20), the piece's masked bytes follow them, and everything in front of the new hold
 * point goes to `write`.  With k = 1 nothing is ever held; a run of bytes < ' ' of any length is held with the bases in front
 * of it.  finish writes what is held.  Both return 0, or 1 when `write` failed (returned non-zero), memory ran out or
 * `back` reaches in front of the held tail; the unit calls nothing but `write`, malloc and free. */
typedef int (*GT4MaskWrite) (const void *bytes, size_t n, void *arg);
typedef struct {
  unsigned char *held;
  size_t n, cap;
  GT4MaskWrite write;
  void *arg;
  int soft;
  unsigned char mask_byte;
} GT4MaskTail;
void gt4_mask_tail_init (GT4MaskTail *t, int soft, unsigned char mask_byte, GT4MaskWrite write, void *arg);
int gt4_mask_tail_push (GT4MaskTail *t, const unsigned char *masked, size_t len, unsigned int back, unsigned int k);
int gt4_mask_tail_finish (GT4MaskTail *t);

/* Device list (NULL with n_words 0: a header alone) -> "<final_name>.tmp" -> rename.  `prefix` ("Error: " or "") goes
 * before the two messages the reference words differently per tool: "Cannot create output file", "Cannot rename".
 * 0: written and renamed; 1: failed after a message, no temporary left; 2: written, the rename failed (message
 * printed, "<final_name>.tmp" stays): the caller decides whether that is fatal. */
int gt4_cli_write_list_file (gt4hip_context *ctx, const gt4hip_list *list, unsigned int word_length, uint64_t n_words, uint64_t total_count,
                             const char *final_name, unsigned int mode, const char *prefix);

#endif
