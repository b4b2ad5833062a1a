/*
 * gt4_listfile.h -- GenomeTester4 `.list` files on the host (C).
 *
 * Drop-in for the file-format side of the hot path: the on-disk header of
 * reference src/word-list.h:40-72, its initialiser (src/word-list.c:33-44) and the validating
 * mmap reader of gt4_word_map_new (src/word-map.c:165-241).  A file is a 48-byte (v4.0: 40-byte)
 * little-endian header followed by packed 12-byte records (u64 key + u32 count), ascending by key.
 */
#ifndef GT4_LISTFILE_H
#define GT4_LISTFILE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 'G'<<24 | 'T'<<16 | '4'<<8 | 'C' and ...'I' (src/word-list.c:31, src/word-index.h) */
#define GT4_LIST_CODE_VALUE 0x47543443u
#define GT4_INDEX_CODE_VALUE 0x47543449u

#define GT4_VERSION_MAJOR 4
#define GT4_VERSION_MINOR 2
#define GT4_VERSION_MICRO 16
#define GT4_VERSION_QUALIFIER "stable"

/* struct _GT4ListHeader_4_4, src/word-list.h:61-72: 48 bytes, no padding */
typedef struct {
  uint32_t code;
  uint32_t version_major;
  uint32_t version_minor;
  uint32_t word_length;
  uint64_t n_words;
  uint64_t total_count;
  uint64_t list_start;
  uint32_t word_bytes;
  uint32_t count_bytes;
} GT4ListHeader;

/* gt4_list_header_init, src/word-list.c:33-44: zero, magic, version 4.2, list_start 48, 8 + 4 */
void gt4_list_header_init (GT4ListHeader *hdr, unsigned int word_length);

/* A list file mapped read-only (the GT4WordMap of the GPU path: records are then uploaded). */
typedef struct {
  char *filename;
  const unsigned char *file_map; /* whole file, PROT_READ / MAP_PRIVATE (src/utils.c:54) */
  uint64_t file_size;
  GT4ListHeader header;          /* normalised as src/word-map.c:198-209 */
  const unsigned char *records;  /* file_map + header.list_start; NULL for a GT4I index file */
  /* GT4I index files (gt4_indexfile_open): the k-mer table of 16-byte (word, first location) entries;
   * the count of entry i is the distance to the next entry's first location, the last one's to
   * index_locations (imap_get_count, src/index-map.c:129-139).  NULL / 0 for list files. */
  const unsigned char *index_kmers;
  uint64_t index_locations;
  /* ... and what --locations, --files and --sequences read: the location section (index_locations packed 64-bit words:
   * file << (n_subseq_bits + n_pos_bits + 1) | sequence << (n_pos_bits + 1) | position << 1 | strand) and the file block
   * (16 bytes "F4TG", two versions, the number of files; then per file size u64, n_sequences u64, name length u16, the
   * name with its NUL, and 28 bytes per sequence).  index_files is NULL and index_n_files 0 for an index without words,
   * which has no file block.  gt4_indexfile_open has walked the block once: the two walkers below stay inside the file. */
  const unsigned char *index_location_words;
  uint32_t index_file_bits, index_subseq_bits, index_pos_bits;
  uint32_t index_n_files;
  const unsigned char *index_files;
} GT4ListFile;

/* struct _GT4IndexHeader, src/index-map.h:69-83: 72 bytes, little-endian, no padding */
typedef struct {
  uint32_t code;
  uint32_t version_major;
  uint32_t version_minor;
  uint32_t word_length;
  uint64_t num_words;
  uint64_t num_locations;
  uint32_t n_file_bits;
  uint32_t n_subseq_bits;
  uint32_t n_pos_bits;
  uint32_t filler0;
  uint64_t files_start;
  uint64_t kmers_start;
  uint64_t locations_start;
} GT4IndexHeader;

enum {
  GT4_LISTFILE_OK = 0,
  GT4_LISTFILE_EOPEN = 1,    /* cannot open / map                                   */
  GT4_LISTFILE_EMAGIC = 2,   /* invalid file tag (src/word-map.c:181)               */
  GT4_LISTFILE_EVERSION = 3, /* incompatible major version (src/word-map.c:185)     */
  GT4_LISTFILE_ESIZE = 4     /* file size too small (src/word-map.c:211-215) -- and headers that pass that test while
                              * the records cannot lie in the file at stride 12: list_start > size or
                              * n_words > (size - list_start) / 12, checked by division (the reference's product wraps);
                              * for an index: any section, or any step through the file block, that leaves the file */
};

/* Reads the 4-byte tag of a file (glistcompare's format sniff, src/glistcompare.c:256-263).
 * Returns 0 and the tag, or 1 when the file cannot be opened / is shorter than 4 bytes. */
int gt4_listfile_sniff (const char *path, uint32_t *code);

/* Maps and validates `path`.  On failure prints the reference's diagnostic to stderr
 * ("gt4_word_map_new: ...") and returns a GT4_LISTFILE_E* code. */
int gt4_listfile_open (const char *path, unsigned int major_version, GT4ListFile *out);
void gt4_listfile_close (GT4ListFile *lf);

/* Maps a GT4I index file (gt4_index_map_new, src/index-map.c:317-373) as a sorted k-mer list: fills
 * header.word_length / n_words (= num_words) / total_count (= num_locations), index_kmers and
 * index_locations; records stays NULL.  The reference checks tag and major version only
 * ("gt4_index_map_new: ..." diagnostics, reproduced); a k-mer table that does not fit in the file
 * is rejected here with GT4_LISTFILE_ESIZE instead of being read out of bounds.  So is everything else a reader of the
 * index follows: locations_start > size or num_locations > (size - locations_start) / 8 (by division), bit sizes with
 * n_file_bits + n_subseq_bits + n_pos_bits + 1 > 64, and a file block that leaves the file anywhere: its 16-byte head,
 * a file's 16 bytes and 2-byte name length, a name (which must end in its NUL), n_sequences x 28 bytes. */
int gt4_indexfile_open (const char *path, unsigned int major_version, GT4ListFile *out);

/* File i (< index_n_files) of a mapped index (index_map_get_file, src/index-map.c:210-230) and sequence j
 * (< n_sequences) of it (index_map_get_sequence, :232-247).  GT4_LISTFILE_OK, or GT4_LISTFILE_ESIZE for an i or j that
 * is not there. */
typedef struct {
  uint64_t size, n_sequences;
  const char *name;                /* NUL-terminated, inside the mapping */
  const unsigned char *sequences;  /* n_sequences x 28 bytes */
} GT4IndexFile;
typedef struct {
  uint64_t name_pos, seq_pos, seq_len;
  uint32_t name_len;
} GT4IndexSequence;
int gt4_indexfile_file (const GT4ListFile *lf, uint32_t i, GT4IndexFile *out);
int gt4_indexfile_sequence (const GT4IndexFile *file, uint64_t j, GT4IndexSequence *out);

/* Incremental writer: placeholder header, records, back-patched header (the reference's
 * fopen/fwrite/fseek sequence, src/glistcompare.c:816-834, :907-915, or write/pwrite, :538-595). */
typedef struct {
  int fd;
  GT4ListHeader header;
} GT4ListWriter;

/* Creates (truncates) `path` with `mode` and writes the placeholder header.  Returns 0 / 1. */
int gt4_listwriter_begin (GT4ListWriter *w, const char *path, unsigned int word_length, unsigned int mode);
/* Appends n packed records (does not touch the header totals).  Returns 0 / 1. */
int gt4_listwriter_append (GT4ListWriter *w, const void *records, uint64_t n);
/* Back-patches n_words / total_count and closes.  Returns 0 / 1. */
int gt4_listwriter_finish (GT4ListWriter *w, uint64_t n_words, uint64_t total_count);
/* Closes without finishing (caller unlinks). */
void gt4_listwriter_abort (GT4ListWriter *w);

/* ---- the head of a GT4I index file as glistmaker --index writes it (reference src/glistmaker.c:366-422, :576-626) */

/* one sequence of an input file: byte offsets in the file (name_len is written in 32 bits) */
typedef struct {
  uint64_t name_pos, name_len, seq_pos, seq_len;
} GT4IndexSubseq;

typedef struct {
  const char *name; /* as given on the command line */
  uint64_t size;    /* of the file, bytes */
  uint64_t n_subseqs;
  const GT4IndexSubseq *subseqs;
} GT4IndexInput;

/* The 72-byte header and, when there is a k-mer at all (have_words), the file block behind it, zero-padded to 8 bytes:
 * everything in front of the k-mer section, in malloc'ed memory (*head, *head_bytes; the caller frees it).  The k-mer
 * section (16 bytes a k-mer) and the locations (8 bytes each) follow it in the file.  The two version fields of the file
 * block are written with their upper halves zero (the reference writes four bytes from a two-byte variable there).
 * Without words the header says what write_index_header says for an empty index: one bit per field, every offset 72.
 * Returns nonzero when memory runs out. */
int gt4_index_head_build (unsigned int word_length, int have_words, uint64_t n_kmers, uint64_t n_locations, unsigned int file_bits, unsigned int subseq_bits,
                          unsigned int pos_bits, const GT4IndexInput *inputs, unsigned int n_inputs, void **head, size_t *head_bytes);

#ifdef __cplusplus
}
#endif
#endif
