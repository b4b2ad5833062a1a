/*
 * gt4_listfile.c -- host-side `.list` file access for the GPU glistcompare path (see
 * include/gt4_listfile.h).  Plain C; no GPU code here.
 */
#define _GNU_SOURCE
#include "gt4_listfile.h"

#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

void gt4_list_header_init (GT4ListHeader *hdr, unsigned int word_length)
{
  memset (hdr, 0, sizeof *hdr);
  hdr->code = GT4_LIST_CODE_VALUE;
  hdr->version_major = GT4_VERSION_MAJOR;
  hdr->version_minor = GT4_VERSION_MINOR;
  hdr->word_length = word_length;
  hdr->list_start = sizeof (GT4ListHeader);
  hdr->word_bytes = 8;
  hdr->count_bytes = 4;
}

int gt4_listfile_sniff (const char *path, uint32_t *code)
{
  int fd = open (path, O_RDONLY);
  if (fd < 0) return 1;
  uint32_t c = 0;
  ssize_t got = read (fd, &c, 4);
  close (fd);
  if (got != 4) return 1;
  *code = c;
  return 0;
}

int gt4_listfile_open (const char *path, unsigned int major_version, GT4ListFile *out)
{
  memset (out, 0, sizeof *out);
  int fd = open (path, O_RDONLY);
  struct stat st;
  if (fd < 0 || fstat (fd, &st) < 0) {
    if (fd >= 0) close (fd);
    fprintf (stderr, "gt4_word_map_new: could not mmap file %s\n", path);
    return GT4_LISTFILE_EOPEN;
  }
  const uint64_t size = (uint64_t) st.st_size;
  const unsigned char *map = NULL;
  if (size) {
    map = (const unsigned char *) mmap (NULL, size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (map == MAP_FAILED) map = NULL;
  }
  close (fd);
  if (!map || size < 16) {
    if (map) munmap ((void *) map, size);
    fprintf (stderr, "gt4_word_map_new: could not mmap file %s\n", path);
    return GT4_LISTFILE_EOPEN;
  }
  /* the first 16 bytes are common to every header version */
  uint32_t code, major, minor;
  memcpy (&code, map, 4);
  memcpy (&major, map + 4, 4);
  memcpy (&minor, map + 8, 4);
  if (code != GT4_LIST_CODE_VALUE) {
    fprintf (stderr, "gt4_word_map_new: invalid file tag (%x, should be %x)\n", code, GT4_LIST_CODE_VALUE);
    munmap ((void *) map, size);
    return GT4_LISTFILE_EMAGIC;
  }
  if (major != major_version) {
    fprintf (stderr, "gt4_word_map_new: incompatible major version %u (required %u)\n", major, major_version);
    munmap ((void *) map, size);
    return GT4_LISTFILE_EVERSION;
  }
  GT4ListHeader h;
  memset (&h, 0, sizeof h);
  const size_t avail = size < sizeof h ? (size_t) size : sizeof h;
  if (minor == 0) {
    /* 4.0: 40-byte header, records right after it */
    memcpy (&h, map, avail < 40 ? avail : 40);
    h.list_start = 40;
    h.word_bytes = 8;
    h.count_bytes = 4;
  } else if (minor <= 2) {
    /* 4.1 / 4.2: list_start from the file, 8 + 4 byte records implied */
    memcpy (&h, map, avail < 40 ? avail : 40);
    h.word_bytes = 8;
    h.count_bytes = 4;
  } else {
    memcpy (&h, map, avail);
  }
  /* The reference's own test (src/word-map.c:211-215) multiplies in wrapping 64-bit arithmetic by the FILE's
   * word_bytes + count_bytes (minor > 2) while every reader -- its own included, src/word-map.h:89-99 -- strides 12:
   * a header with n_words = 2^40 and 0 + 0 bytes per record, or with n_words = 2^64 / 12 + 1, passes it and is then
   * read far beyond the mapping.  Here: the reference's test first (same message, same number, where it fires), then
   * the bound that actually protects the readers, by division: list_start inside the file and n_words records of 12
   * bytes behind it. */
  const uint64_t ref_need = h.list_start + h.n_words * (uint64_t) (h.word_bytes + h.count_bytes);
  const int fits = h.list_start <= size && h.n_words <= (size - h.list_start) / 12u;
  if (size < ref_need || !fits) {
    uint64_t need = ref_need;
    if (size >= ref_need) { /* (the reference would have gone on: say what the readers need, saturating) */
      need = h.n_words > (UINT64_MAX - h.list_start) / 12u ? UINT64_MAX : h.list_start + 12u * h.n_words;
      if (h.list_start > size && need < h.list_start) need = h.list_start;
    }
    fprintf (stderr, "gt4_word_map_new: file size too small (%llu, should be at least %llu)\n", (unsigned long long) size,
             (unsigned long long) need);
    munmap ((void *) map, size);
    return GT4_LISTFILE_ESIZE;
  }
  out->filename = strdup (path);
  out->file_map = map;
  out->file_size = size;
  out->header = h;
  out->records = map + h.list_start;
  return GT4_LISTFILE_OK;
}

/* Walks the file block at `at` of a mapping of `size` bytes up to file `want` (~0: to the end), never reading a byte
 * that was not first shown to lie in the file.  0 and *n_files (and *file for `want`), or 1 where a step leaves the file. */
static int file_block_walk (const unsigned char *map, uint64_t size, uint64_t at, uint32_t want, uint32_t *n_files, GT4IndexFile *file)
{
  if (size - at < 16) return 1;
  memcpy (n_files, map + at + 12, 4);
  at += 16;
  for (uint32_t i = 0; i < *n_files; i++) {
    uint64_t fsize, n_seqs;
    uint16_t len;
    if (size - at < 18) return 1;
    memcpy (&fsize, map + at, 8);
    memcpy (&n_seqs, map + at + 8, 8);
    memcpy (&len, map + at + 16, 2);
    at += 18;
    if (len < 1 || size - at < len || map[at + len - 1] != 0) return 1;
    at += len;
    if (n_seqs > (size - at) / 28) return 1;
    if (i == want) {
      file->size = fsize;
      file->n_sequences = n_seqs;
      file->name = (const char *) map + at - len;
      file->sequences = map + at;
      return 0;
    }
    at += n_seqs * 28;
  }
  return want != ~0u;
}

int gt4_indexfile_file (const GT4ListFile *lf, uint32_t i, GT4IndexFile *out)
{
  uint32_t n = 0;
  if (!lf || !out || !lf->index_files || i >= lf->index_n_files) return GT4_LISTFILE_ESIZE;
  return file_block_walk (lf->file_map, lf->file_size, (uint64_t) (lf->index_files - lf->file_map), i, &n, out) ? GT4_LISTFILE_ESIZE : GT4_LISTFILE_OK;
}

int gt4_indexfile_sequence (const GT4IndexFile *file, uint64_t j, GT4IndexSequence *out)
{
  if (!file || !out || j >= file->n_sequences) return GT4_LISTFILE_ESIZE;
  const unsigned char *s = file->sequences + j * 28;
  memcpy (&out->name_pos, s, 8);
  memcpy (&out->name_len, s + 8, 4);
  memcpy (&out->seq_pos, s + 12, 8);
  memcpy (&out->seq_len, s + 20, 8);
  return GT4_LISTFILE_OK;
}

int gt4_indexfile_open (const char *path, unsigned int major_version, GT4ListFile *out)
{
  memset (out, 0, sizeof *out);
  int fd = open (path, O_RDONLY);
  struct stat st;
  if (fd < 0 || fstat (fd, &st) < 0) {
    if (fd >= 0) close (fd);
    fprintf (stderr, "gt4_index_map_new: could not mmap file %s\n", path);
    return GT4_LISTFILE_EOPEN;
  }
  const uint64_t size = (uint64_t) st.st_size;
  const unsigned char *map = NULL;
  if (size) {
    map = (const unsigned char *) mmap (NULL, size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (map == MAP_FAILED) map = NULL;
  }
  close (fd);
  if (!map || size < sizeof (GT4IndexHeader)) {
    if (map) munmap ((void *) map, size);
    fprintf (stderr, "gt4_index_map_new: could not mmap file %s\n", path);
    return GT4_LISTFILE_EOPEN;
  }
  GT4IndexHeader h;
  memcpy (&h, map, sizeof h);
  if (h.code != GT4_INDEX_CODE_VALUE) {
    fprintf (stderr, "gt4_index_map_new: invalid file tag (%x, should be %x)\n", h.code, GT4_INDEX_CODE_VALUE);
    munmap ((void *) map, size);
    return GT4_LISTFILE_EMAGIC;
  }
  if (h.version_major != major_version) {
    fprintf (stderr, "gt4_index_map_new: incompatible major version %u (required %u)\n", h.version_major, major_version);
    munmap ((void *) map, size);
    return GT4_LISTFILE_EVERSION;
  }
  if (h.kmers_start > size || h.num_words > (size - h.kmers_start) / 16) {
    fprintf (stderr, "gt4_index_map_new: file size too small (%llu) for %llu k-mers at %llu\n", (unsigned long long) size,
             (unsigned long long) h.num_words, (unsigned long long) h.kmers_start);
    munmap ((void *) map, size);
    return GT4_LISTFILE_ESIZE;
  }
  if (h.locations_start > size || h.num_locations > (size - h.locations_start) / 8) {
    fprintf (stderr, "gt4_index_map_new: file size too small (%llu) for %llu locations at %llu\n", (unsigned long long) size,
             (unsigned long long) h.num_locations, (unsigned long long) h.locations_start);
    munmap ((void *) map, size);
    return GT4_LISTFILE_ESIZE;
  }
  if (h.n_file_bits > 64 || h.n_subseq_bits > 64 || h.n_pos_bits > 64 || h.n_file_bits + h.n_subseq_bits + h.n_pos_bits + 1 > 64) {
    fprintf (stderr, "gt4_index_map_new: a location of %u + %u + %u + 1 bits does not fit 64\n", h.n_file_bits, h.n_subseq_bits, h.n_pos_bits);
    munmap ((void *) map, size);
    return GT4_LISTFILE_ESIZE;
  }
  /* an index without words ends behind its header (files_start = size): it has no file block */
  uint32_t n_files = 0;
  if (h.files_start > size || (h.files_start < size && file_block_walk (map, size, h.files_start, ~0u, &n_files, NULL))) {
    fprintf (stderr, "gt4_index_map_new: file size too small (%llu) for the file block at %llu\n", (unsigned long long) size,
             (unsigned long long) h.files_start);
    munmap ((void *) map, size);
    return GT4_LISTFILE_ESIZE;
  }
  out->filename = strdup (path);
  out->file_map = map;
  out->file_size = size;
  out->index_location_words = map + h.locations_start;
  out->index_file_bits = h.n_file_bits;
  out->index_subseq_bits = h.n_subseq_bits;
  out->index_pos_bits = h.n_pos_bits;
  out->index_n_files = n_files;
  out->index_files = h.files_start < size ? map + h.files_start : NULL;
  gt4_list_header_init (&out->header, h.word_length);
  out->header.n_words = h.num_words;
  out->header.total_count = h.num_locations;
  out->records = NULL;
  out->index_kmers = map + h.kmers_start;
  out->index_locations = h.num_locations;
  return GT4_LISTFILE_OK;
}

void gt4_listfile_close (GT4ListFile *lf)
{
  if (!lf) return;
  if (lf->file_map) munmap ((void *) lf->file_map, lf->file_size);
  free (lf->filename);
  memset (lf, 0, sizeof *lf);
}

static int write_all (int fd, const void *buf, size_t len)
{
  const char *p = (const char *) buf;
  while (len) {
    ssize_t w = write (fd, p, len);
    if (w < 0) {
      if (errno == EINTR) continue;
      return 1;
    }
    p += w;
    len -= (size_t) w;
  }
  return 0;
}

int gt4_listwriter_begin (GT4ListWriter *w, const char *path, unsigned int word_length, unsigned int mode)
{
  gt4_list_header_init (&w->header, word_length);
  w->fd = open (path, O_WRONLY | O_CREAT | O_TRUNC, (mode_t) mode);
  if (w->fd < 0) return 1;
  return write_all (w->fd, &w->header, sizeof w->header);
}

int gt4_listwriter_append (GT4ListWriter *w, const void *records, uint64_t n)
{
  return write_all (w->fd, records, (size_t) n * 12u);
}

int gt4_listwriter_finish (GT4ListWriter *w, uint64_t n_words, uint64_t total_count)
{
  w->header.n_words = n_words;
  w->header.total_count = total_count;
  int bad = pwrite (w->fd, &w->header, sizeof w->header, 0) != (ssize_t) sizeof w->header;
  bad |= close (w->fd) != 0;
  w->fd = -1;
  return bad;
}

void gt4_listwriter_abort (GT4ListWriter *w)
{
  if (w->fd >= 0) close (w->fd);
  w->fd = -1;
}

/* ---- GT4I index: header + file block */

static unsigned char *put_u16 (unsigned char *p, unsigned int v) { p[0] = (unsigned char) v, p[1] = (unsigned char) (v >> 8); return p + 2; }
static unsigned char *put_u32 (unsigned char *p, uint32_t v) { memcpy (p, &v, 4); return p + 4; }
static unsigned char *put_u64 (unsigned char *p, uint64_t v) { memcpy (p, &v, 8); return p + 8; }

int gt4_index_head_build (unsigned int word_length, int have_words, uint64_t n_kmers, uint64_t n_locations, unsigned int file_bits, unsigned int subseq_bits,
                          unsigned int pos_bits, const GT4IndexInput *inputs, unsigned int n_inputs, void **head, size_t *head_bytes)
{
  size_t block = 0;
  if (have_words) {
    block = 16;
    for (unsigned int i = 0; i < n_inputs; i++) block += 18 + strlen (inputs[i].name) + 1 + (size_t) inputs[i].n_subseqs * 28;
    block = (block + 7) & ~(size_t) 7;
  }
  unsigned char *b = (unsigned char *) calloc (1, 72 + block), *p = b;
  if (!b) return 1;
  memcpy (p, "I4TG", 4);
  p = put_u32 (p + 4, 4);
  p = put_u32 (p, 2);
  p = put_u32 (p, word_length);
  p = put_u64 (p, have_words ? n_kmers : 0);
  p = put_u64 (p, have_words ? n_locations : 0);
  p = put_u32 (p, have_words ? file_bits : 1);
  p = put_u32 (p, have_words ? subseq_bits : 1);
  p = put_u32 (p, have_words ? pos_bits : 1);
  p = put_u32 (p, 0);
  p = put_u64 (p, 72);
  p = put_u64 (p, 72 + block);
  p = put_u64 (p, 72 + block + (have_words ? n_kmers * 16 : 0));
  if (have_words) {
    memcpy (p, "F4TG", 4);
    p = put_u32 (p + 4, 4);
    p = put_u32 (p, 2);
    p = put_u32 (p, n_inputs);
    for (unsigned int i = 0; i < n_inputs; i++) {
      const size_t len = strlen (inputs[i].name) + 1;
      p = put_u64 (p, inputs[i].size);
      p = put_u64 (p, inputs[i].n_subseqs);
      p = put_u16 (p, (unsigned int) len);
      memcpy (p, inputs[i].name, len);
      p += len;
      for (uint64_t j = 0; j < inputs[i].n_subseqs; j++) {
        const GT4IndexSubseq *s = &inputs[i].subseqs[j];
        p = put_u64 (p, s->name_pos);
        p = put_u32 (p, (uint32_t) s->name_len);
        p = put_u64 (p, s->seq_pos);
        p = put_u64 (p, s->seq_len);
      }
    }
  }
  *head = b;
  *head_bytes = 72 + block;
  return 0;
}
