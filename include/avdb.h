/*
 * avdb.h — C ABI of libavdb_hip.so, the MI355X (gfx950) kernel library behind
 * the AnnotatedVDB batch variant -> genomic-bin / primary-key path.
 *
 * Plain C: no torch or HIP types in any signature.  Every entry point returns
 * an int status (AVDB_OK == 0; negative on failure, message via
 * avdb_last_error()).  Array arguments are DEVICE pointers (HBM) unless marked
 * "host"; the caller owns every buffer.  `stream` is a hipStream_t passed as
 * void* (NULL = the device's null stream); all device work is enqueued on it
 * and nothing synchronises, so callers may capture the calls into a hipGraph.
 *
 * Reference interfaces replaced (paths relative to NIAGADS/AnnotatedVDB):
 *   - BinIndex.find_bin_index(chrm, start, end=None)      BinIndex/lib/python/bin_index.py:59-75
 *     and the external SQL find_bin_index(chr,start,end) it calls through
 *     BIN_INDEX_SQL (bin_index.py:9-14, _update_current_bin_index :43-56)
 *   - the BinIndexRef table it searches        BinIndex/bin/generate_bin_index_references.py:46-83
 *   - VariantAnnotator.infer_variant_end_location  Util/lib/python/variant_annotator.py:36-79
 *     and __normalize_alleles (common-prefix trim)  variant_annotator.py:82-121
 *   - VariantPKGenerator.generate_primary_key / compute_vrs_identifier
 *                                               Util/lib/python/primary_key_generator.py:99-165
 *   - the per-alt record-prep loop              Util/lib/python/loaders/vcf_variant_loader.py:259-348
 *   - in-batch duplicate-key semantics          Load/lib/sql/annotatedvdb_schema/patches/removeDuplicates.sql:2-24
 *
 * Record layout (structure of arrays, one entry per alt allele):
 *   chrom      u8[n]   contig code, index into the context's chromosome table
 *                      (default order chr1..chr22, chrX, chrY, chrM —
 *                      Util/lib/python/enums/chromosomes.py:9-38)
 *   pos/start  u32[n]  1-based VCF POS
 *   end        u32[n]  1-based inclusive end (nullable => end = start, bin_index.py:63)
 *   allele_off u64[n]  byte offset of the REF allele in `heap`; ALT follows at
 *                      allele_off + ref_len (raw, un-normalised VCF bytes)
 *   ref_len    u32[n], alt_len u32[n]
 *   ext_id     u64[n]  external id key (refSNP); 0 = none; equal keys <=> equal ids
 *   heap_bytes         size of the heap allocation: kernels read allele bytes as
 *                      8-byte-aligned words and never touch memory outside
 *                      [heap, heap + heap_bytes)
 *
 * Bin code (u32): level in bits 31..28 (0 = whole chromosome .. 13 = 15,625 bp
 * leaf), 0-based index of the bin at that level in bits 27..0.  The ltree path
 * "chrN.L1.B<k>...L<level>.B<k>" is a pure function of (chrom, code):
 * avdb_format_bin_path().  AVDB_BIN_NONE marks an unmappable record (the
 * reference raises TypeError there, bin_index.py:75).
 */
#ifndef AVDB_H_
#define AVDB_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: avdb_format_opts gained struct_size (first field) and adsp_dup; K5h/K8h/K1h
 *    host entries; AVDB_KEY_OVERFLOW / AVDB_PATH_OVERFLOW key states */
#define AVDB_ABI_VERSION 2

/* return codes */
#define AVDB_OK 0
#define AVDB_EINVAL (-1)   /* bad argument (null ctx, n too large, misaligned ...) */
#define AVDB_EHIP (-2)     /* HIP runtime error (launch / allocation) */
#define AVDB_ENOMEM (-3)
#define AVDB_ERANGE (-4)   /* output buffer too small */
#define AVDB_ERCCL (-5)    /* RCCL could not be loaded, or a collective failed */
#define AVDB_ENOTBGZF (-6) /* avdb_bgzf_index_host: the first member is gzip, but not BGZF */

/* per-record status (u8) */
#define AVDB_STATUS_OK 0
#define AVDB_STATUS_UNKNOWN_CHROM 1
#define AVDB_STATUS_OUT_OF_RANGE 2      /* start < 1 or end > chromosome length */
#define AVDB_STATUS_END_BEFORE_START 3  /* bin of [end,start]; reference answer is cache-history dependent */

#define AVDB_BIN_NONE 0xFFFFFFFFu
#define AVDB_N_LEVELS 14
#define AVDB_MAX_CHROM 64
#define AVDB_DIGEST_CHARS 32            /* sha512t24u: 24 bytes, base64url, no padding */
#define AVDB_MAX_PATH 128

/* counters[] slots (u64, accumulated) written by avdb_bin_assign / avdb_record_prep
 * (records, per-status) and avdb_pk_dedup / avdb_vrs_digest (dup/collision/long);
 * slots [0..15] are reserved */
#define AVDB_CTR_STATUS0 16             /* [16..19]: records per status */
#define AVDB_CTR_RECORDS 20
#define AVDB_CTR_DUPLICATES 21          /* records whose primary key repeats an earlier one */
#define AVDB_CTR_HASH_COLLISIONS 22     /* fingerprint collisions resolved by byte compare */
#define AVDB_CTR_LONG 23                /* records with ref_len + alt_len > max_seq_len */
#define AVDB_CTR_COPY_ROWS 24           /* COPY rows written by avdb_vcf_format_write */
#define AVDB_CTR_SKIPPED_ALTS 25        /* ALT '.' entries skipped (vcf_variant_loader.py:277-280) */
#define AVDB_CTR_DUP_ROWS 26            /* records whose COPY row was dropped (keep == 0) */
#define AVDB_CTR_HOST_LINES 27          /* lines left to the host renderer */
#define AVDB_CTR_EXISTING 28            /* records found in the existing-variant key set (K6) */
#define AVDB_CTR_ADSP_UPDATES 29        /* ADSP records whose key was already loaded (is_adsp_variant UPDATEs) */
#define AVDB_N_COUNTERS 32

typedef struct avdb_ctx avdb_ctx;

int avdb_abi_version(void);
/* Thread-local description of the last failure in this thread. */
const char* avdb_last_error(void);
int avdb_device_count(int* n);

/* ---- context -----------------------------------------------------------
 * One context per device.  chrom_len (host) gives each contig's length; it is
 * the information BinIndexRef carries (generate_bin_index_references.py:17-43).
 * Not thread-safe per context; calls are ordered on the caller's stream.  */
int avdb_ctx_create(int device, const uint32_t* chrom_len_host, int n_chrom, avdb_ctx** out);
int avdb_ctx_destroy(avdb_ctx* ctx);
/* Launch-shape options of a context (same results, another grid):
 *   AVDB_OPT_K4_GRID  workgroups of K4's persistent digest grid, 0 = its occupancy on
 *                     every CU (the default); fewer leave CUs to K7 running beside K4
 *                     on another stream (AVDB_KEYS_DIGEST_DEFERRED).
 */
#define AVDB_OPT_K4_GRID 1
/*   AVDB_OPT_K7_GRID  workgroups (one wave each) of K7's write pass, 0 = the default; a
 *                     persistent grid below the chip's occupancy leaves registers to K4 */
#define AVDB_OPT_K7_GRID 2
/*   AVDB_OPT_K11_GRID workgroups (one wave each) of K11's inflate grid, 0 = sixteen per CU; at most
 *                     16384; fewer make each stride over more members */
#define AVDB_OPT_K11_GRID 3
int avdb_ctx_set_option(avdb_ctx* ctx, int option, int64_t value);
int avdb_ctx_n_chrom(const avdb_ctx* ctx);
/* GA4GH refget digests (32 chars each, no "ga4gh:SQ." prefix) of every contig,
 * host array n_chrom*32 bytes; required only by avdb_vrs_digest. */
int avdb_ctx_set_sequence_digests(avdb_ctx* ctx, const char* digests_host, int n_chrom);
/* Number of L8 (500 kb) bins over the whole chromosome table (histogram size). */
int avdb_l8_bin_count(const avdb_ctx* ctx, uint32_t* n_bins);

/* ---- K1: smallest enclosing bin ----------------------------------------
 * Replaces BinIndex.find_bin_index + SQL find_bin_index (bin_index.py:43-75).
 * end may be NULL (end = start); status may be NULL.  If hist_l8 (u32[n_l8])
 * and/or counters (u64[AVDB_N_COUNTERS]) are non-NULL they are ACCUMULATED
 * (caller zeroes them): L8 bin of `start` for every mappable record, records
 * and records per status. */
int avdb_bin_assign(avdb_ctx* ctx, const uint8_t* chrom, const uint32_t* start,
                    const uint32_t* end, size_t n, uint32_t* bin_code, uint8_t* status,
                    uint32_t* hist_l8, uint64_t* counters, void* stream);

/* ---- K2: record prep (end inference + bin, fused) ------------------------
 * Per alt allele: common-prefix length of ref/alt (variant_annotator.py:82-121),
 * inferred end (variant_annotator.py:36-79), then the bin of [pos,end]
 * (vcf_variant_loader.py:310-311).  end_out/bin_code required; status, lcp,
 * hist_l8, counters optional (NULL).  */
int avdb_record_prep(avdb_ctx* ctx, const uint8_t* chrom, const uint32_t* pos,
                     const uint64_t* allele_off, const uint32_t* ref_len, const uint32_t* alt_len,
                     const uint8_t* heap, size_t heap_bytes, size_t n, uint32_t* end_out,
                     uint32_t* bin_code,
                     uint8_t* status, uint32_t* lcp, uint32_t* hist_l8, uint64_t* counters,
                     void* stream);

/* ---- K3: in-batch primary-key dedup --------------------------------------
 * keep[i] = 1 iff no j < i has the same primary key chr:pos:ref:alt[:ext]
 * (primary_key_generator.py:99-122; equal keys <=> equal (chrom,pos,ref,alt,ext_id)).
 * grouped != 0 promises records with equal (chrom,pos) are contiguous (any
 * position-sorted VCF): a run scan; a 16-byte-aligned `workspace` of at least
 * 16384 + 4*round_up(n, 4) bytes (optional) lets it list the records that share
 * their predecessor's position and resolve only those (faster).  grouped == 0: hash
 * path, needs `workspace` of avdb_pk_dedup_workspace_size() bytes (device).
 * counters[AVDB_CTR_DUPLICATES / _HASH_COLLISIONS] accumulated if non-NULL. */
int avdb_pk_dedup_workspace_size(size_t n, size_t* bytes);
int avdb_pk_dedup(avdb_ctx* ctx, const uint8_t* chrom, const uint32_t* pos,
                  const uint64_t* allele_off, const uint32_t* ref_len, const uint32_t* alt_len,
                  const uint8_t* heap, size_t heap_bytes, const uint64_t* ext_id, size_t n,
                  int grouped,
                  void* workspace, size_t workspace_bytes, uint8_t* keep, uint64_t* counters,
                  void* stream);
/* The same (grouped, list form) with flags: AVDB_DEDUP_MARKED = avdb_record_prep_keyed
 * already ran the first phase for this batch (keep = 1 everywhere, the records that
 * share their predecessor's position listed in `workspace`, which must be the one it
 * was given, with `keep` its keep array): only the run scan over those lists runs. */
#define AVDB_DEDUP_MARKED 1u
/* With AVDB_DEDUP_MARKED: the marks came from avdb_keyed_prep (its list layout). */
#define AVDB_DEDUP_ONEPASS 2u
int avdb_pk_dedup_ex(avdb_ctx* ctx, const uint8_t* chrom, const uint32_t* pos, const uint64_t* allele_off,
                     const uint32_t* ref_len, const uint32_t* alt_len, const uint8_t* heap, size_t heap_bytes,
                     const uint64_t* ext_id, size_t n, void* workspace, size_t workspace_bytes, uint8_t* keep,
                     uint64_t* counters, uint32_t flags, void* stream);

/* ---- K4: digests ---------------------------------------------------------
 * sha512t24u of n byte strings (data + off[i], len[i]) -> out[i*32..] base64url. */
int avdb_sha512t24u(avdb_ctx* ctx, const uint8_t* data, const uint64_t* off, const uint32_t* len,
                    size_t n, char* out, void* stream);
/* Long-allele key digest (compute_vrs_identifier, primary_key_generator.py:147-165):
 * for every record with ref_len + alt_len > max_seq_len, the VRS-1.x Allele
 * digest of interval (pos-1, pos-1+ref_len] and literal state ALT, written to
 * digest_out[i*32..] (other rows untouched); is_long[i] set 0/1 if non-NULL.
 * Long rows are compacted into `workspace` (avdb_vrs_digest_workspace_size()
 * bytes, device, 16-byte aligned) first.  PARITY UNPINNED. */
int avdb_vrs_digest_workspace_size(size_t n, size_t* bytes);
int avdb_vrs_digest(avdb_ctx* ctx, const uint8_t* chrom, const uint32_t* pos,
                    const uint64_t* allele_off, const uint32_t* ref_len, const uint32_t* alt_len,
                    const uint8_t* heap, size_t heap_bytes, size_t n, uint32_t max_seq_len,
                    void* workspace,
                    size_t workspace_bytes, char* digest_out, uint8_t* is_long, void* stream);
/* The same with flags: AVDB_DIGEST_CODES_READY = avdb_record_prep_keyed already
 * classified this batch's records into the workspace (same n and max_seq_len), so
 * the pass over both length arrays is replaced by one over those bytes. */
#define AVDB_DIGEST_CODES_READY 1u
int avdb_vrs_digest_ex(avdb_ctx* ctx, const uint8_t* chrom, const uint32_t* pos, const uint64_t* allele_off,
                       const uint32_t* ref_len, const uint32_t* alt_len, const uint8_t* heap, size_t heap_bytes,
                       size_t n, uint32_t max_seq_len, void* workspace, size_t workspace_bytes, char* digest_out,
                       uint8_t* is_long, uint32_t flags, void* stream);
/* The same, and every long record's 32 characters also written into the key text
 * of a deferred K7 / avdb_keyed_prep call on the same batch (key_off / key_out /
 * key_state: that call's; the keys in state AVDB_KEY_DIGEST_PENDING get them at
 * key_off[i] + len("label:pos:") and become AVDB_KEY_OK) — the work of
 * avdb_primary_keys_fill_digests without its pass over every record. */
int avdb_vrs_digest_keys(avdb_ctx* ctx, const uint8_t* chrom, const uint32_t* pos, const uint64_t* allele_off,
                         const uint32_t* ref_len, const uint32_t* alt_len, const uint8_t* heap, size_t heap_bytes,
                         size_t n, uint32_t max_seq_len, void* workspace, size_t workspace_bytes, char* digest_out,
                         uint8_t* is_long, uint32_t flags, const uint64_t* key_off, uint8_t* key_out,
                         uint8_t* key_state, void* stream);

/* ---- K0: VCF text -> per-alt record SoA ----------------------------------
 * Replaces the text half of VcfEntryParser.parse_entry / get_variant / get_refsnp
 * (Util/lib/python/parsers/vcf_parser.py:76-169) and the per-alt loop head of
 * VCFVariantLoader.__parse_alt_alleles (vcf_variant_loader.py:273-280) for a batch
 * of VCF lines resident in device memory (`text`, '\n'-separated, as
 * load_vcf_file.py:101-119 reads them; each line is rstripped).
 *   1. avdb_vcf_count_lines  -> number of '\n' bytes (device u64); the caller derives
 *      n_lines = n_newlines + (text does not end in '\n').
 *   2. avdb_vcf_parse_lines  -> one avdb_vcf_line per line, plus exclusive prefix sums
 *      rec_off[n_lines+1] / heap_off[n_lines+1] of records and allele-heap bytes.
 *      `line_counts` is the workspace step 1 filled (its per-workgroup newline
 *      offsets are reused); NULL recounts.
 *   3. avdb_vcf_emit         -> the record SoA K2/K3/K4 consume (one row per ALT that
 *      is not '.', REF+ALT copied into `heap`), with rec_line/rec_alt back-references.
 * Text cases the GPU does not canonicalise are flagged for the host (flags below). */
#define AVDB_VCF_COMMENT 0x001u         /* starts with '#': not a data line */
#define AVDB_VCF_FEW_FIELDS 0x002u      /* < 8 tab-separated fields (IndexError, vcf_parser.py:98-100) */
#define AVDB_VCF_BAD_POS 0x004u         /* POS not a plain decimal < 2^32: host resolves */
#define AVDB_VCF_EXT_HOST 0x008u        /* refSNP id not canonical rs<N>: host interns ext_id */
#define AVDB_VCF_ID_RS 0x010u           /* 'rs' in ID: ref_snp_id = ID (vcf_parser.py:164) */
#define AVDB_VCF_INFO_RS 0x020u         /* ref_snp_id = 'rs' + INFO RS (vcf_parser.py:166-167) */
#define AVDB_VCF_ID_METASEQ 0x040u      /* ID is '.' or starts 'rs': variant id = chr:pos:ref:alt (:140-142) */
#define AVDB_VCF_CHROM_HOST 0x080u      /* CHROM has non-alphanumeric bytes: host resolves */
#define AVDB_VCF_EMPTY 0x100u           /* empty after rstrip */
#define AVDB_VCF_ID_HOST 0x200u         /* ID looks numeric (Python coerces it): host resolves */

typedef struct avdb_vcf_line {
  uint64_t start;         /* byte offset of the line in text */
  uint32_t len;           /* bytes after rstrip */
  uint32_t n_fields;      /* tab-separated fields */
  uint32_t field[8];      /* start of fields 0..7 relative to `start` (field k ends at field[k+1]-1) */
  uint32_t field_end8;    /* end of field 7 (INFO) relative to `start` */
  uint32_t pos;
  uint64_t ext_id;
  uint32_t n_alt;         /* ALT entries including '.' */
  uint32_t n_rec;         /* records emitted (ALT != '.') */
  uint32_t flags;
  uint8_t chrom;          /* contig code, 255 unknown */
  uint8_t pad[3];
} avdb_vcf_line;

#define AVDB_VCF_COUNT_WORKSPACE_BYTES 32768u /* minimum workspace of avdb_vcf_count_lines */
int avdb_vcf_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes);
/* Workspace of avdb_vcf_count_lines that also holds the newline count of every
 * parse window (AVDB_VCF_PARSE_WIN_KB pieces of the count pass's cut, 24 KB by
 * default): given that much, the count
 * pass writes them and avdb_vcf_parse_lines2 parses one window per workgroup,
 * finding the line starts itself, with no separate line-starts pass.  With only
 * AVDB_VCF_COUNT_WORKSPACE_BYTES the starts pass runs (same outputs). */
int avdb_vcf_count_workspace_size(size_t text_bytes, size_t* bytes);
int avdb_vcf_count_lines(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, void* workspace,
                         size_t workspace_bytes, uint64_t* n_newlines, void* stream);
/* Parse options (nullable = the default 8-field header, no chromosome map):
 *   min_fields  the loader's header width (VCFVariantLoader.set_vcf_header_fields,
 *               vcf_variant_loader.py:88-93,368, for a header whose first eight fields are
 *               the standard ones, e.g. a pVCF): a line with fewer values is flagged
 *               AVDB_VCF_FEW_FIELDS (the reference raises IndexError there);
 *   chrom_map   VcfEntryParser.update_chromosome (vcf_parser.py:117-124) with a
 *               ChromosomeMap (chromosome_map_parser.py:84-91): CHROM is looked up as
 *               bytes; a CHROM not in the map, or mapped to a key the host must
 *               resolve, is flagged AVDB_VCF_CHROM_HOST (the reference raises KeyError). */
typedef struct avdb_chrom_map avdb_chrom_map;
typedef struct avdb_vcf_opts {
  uint32_t struct_size;             /* sizeof(avdb_vcf_opts) */
  uint32_t min_fields;
  const avdb_chrom_map* chrom_map;  /* nullable */
} avdb_vcf_opts;
/* keys (host): the map's source ids, keys[key_off[k] .. key_off[k+1]); codes[k] (host):
 * the contig code of the chromosome source id k maps to, 0xFF = lines with this CHROM
 * are rendered by the caller.  The first of duplicate keys wins. */
int avdb_chrom_map_create(avdb_ctx* ctx, const uint8_t* keys_host, const uint64_t* key_off_host, size_t n_keys,
                          const uint8_t* codes_host, avdb_chrom_map** out);
int avdb_chrom_map_destroy(avdb_chrom_map* map);
int avdb_vcf_parse_lines(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                         const void* line_counts, void* workspace, size_t workspace_bytes,
                         avdb_vcf_line* lines,
                         uint64_t* rec_off, uint64_t* heap_off, const avdb_vcf_opts* opts, void* stream);
/* avdb_vcf_parse_lines with the size of `line_counts`: a count workspace of at
 * least avdb_vcf_count_workspace_size(text_bytes) bytes takes the window path. */
/* `lines` may be NULL here: no public line table is written (the tokenize-only
 * path), and what the emit needs of each line (32 bytes) goes into `workspace`
 * instead, for avdb_vcf_emit_ws with that same workspace. */
int avdb_vcf_parse_lines2(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                          const void* line_counts, size_t line_counts_bytes, void* workspace,
                          size_t workspace_bytes, avdb_vcf_line* lines, uint64_t* rec_off, uint64_t* heap_off,
                          const avdb_vcf_opts* opts, void* stream);
int avdb_vcf_emit(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                  const avdb_vcf_line* lines, const uint64_t* rec_off, const uint64_t* heap_off,
                  uint8_t* chrom, uint32_t* pos, uint64_t* allele_off, uint32_t* ref_len,
                  uint32_t* alt_len, uint64_t* ext_id, uint8_t* heap, uint32_t* rec_line,
                  uint32_t* rec_alt, void* stream);
/* avdb_vcf_emit after avdb_vcf_parse_lines2(..., lines = NULL, ...): the line data
 * comes from that call's workspace (same text_bytes and n_lines). */
int avdb_vcf_emit_ws(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                     const void* parse_workspace, size_t parse_workspace_bytes, const uint64_t* rec_off,
                     const uint64_t* heap_off, uint8_t* chrom, uint32_t* pos, uint64_t* allele_off,
                     uint32_t* ref_len, uint32_t* alt_len, uint64_t* ext_id, uint8_t* heap, uint32_t* rec_line,
                     uint32_t* rec_alt, void* stream);
/* The records without the count pass (the tokenize-only path, no line table):
 * avdb_vcf_parse_local parses one workgroup per parse window with no line numbers
 * known, each window writing its lines' counts, its records and their REF+ALT bytes
 * to slots of its own in `workspace` (avdb_vcf_local_workspace_size(text_bytes)
 * bytes, 16-byte aligned), from the text it has staged; one scan of the windows'
 * totals then gives every window its first line, record and heap byte.
 * totals (device, 4 x u64): lines, records, heap bytes, and the number of windows
 * the path could not take (more than AVDB_VCF_LOCAL_CAP = 1024 lines or records in
 * a 24 KB window, more than 24 KB of REF+ALT bytes in its records, or a line whose
 * records / heap bytes exceed 2^23).  With totals[3] == 0, avdb_vcf_emit_local moves
 * the slots into the same records, heap, rec_line / rec_alt and per-line rec_off /
 * heap_off (totals[0] + 1 entries each, nullable) as count -> parse ->
 * avdb_vcf_emit_ws write — coalesced copies; it does not read the text (`text` is
 * kept in the signature and may be NULL); with totals[3] != 0 the caller takes that
 * counted path.  The same workspace goes to both calls.  Workspace per 24 KB window
 * of text: 1,024 line slots of 8 bytes, 1,024 record slots of 32 bytes, 24 KB of
 * heap slots and 40 bytes of window totals, about 2.7x text_bytes at any size (a
 * one-line text: two windows, 128 KB); the slots are written only for the lines
 * and records present. */
int avdb_vcf_local_workspace_size(size_t text_bytes, size_t* bytes);
int avdb_vcf_parse_local(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, void* workspace,
                         size_t workspace_bytes, const avdb_vcf_opts* opts, uint64_t* totals, void* stream);
int avdb_vcf_emit_local(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, const void* workspace,
                        size_t workspace_bytes, uint64_t* rec_off, uint64_t* heap_off, uint8_t* chrom, uint32_t* pos,
                        uint64_t* allele_off, uint32_t* ref_len, uint32_t* alt_len, uint64_t* ext_id, uint8_t* heap,
                        uint32_t* rec_line, uint32_t* rec_alt, void* stream);

/* ---- K5: the load driver's text outputs ---------------------------------
 * Replaces the per-alt COPY row assembly of VCFVariantLoader.__parse_alt_alleles
 * (vcf_variant_loader.py:320-343) — primary key (primary_key_generator.py:99-122),
 * metaseq id, bin path, refSNP, multi-allelic flag, display attributes
 * (variant_annotator.py:134-241) and INFO FREQ allele frequencies
 * (vcf_parser.py:200-222), both as json.dumps text — and the .mapping line
 * (Load/bin/load_vcf_file.py:116-117), for lines K0 tokenized and K2 (end,
 * bin_code, status), K4 (digest, long keys; NULL if none) and K3 (keep; NULL =
 * keep all) processed.
 *   1. avdb_vcf_format_size : line_state[n_lines] and exclusive byte offsets
 *      copy_off[n_lines+1] / map_off[n_lines+1] (totals in [n_lines]);
 *      workspace of avdb_format_workspace_size(n_lines) bytes.
 *   2. avdb_vcf_format_write: the texts into copy_out / map_out (8-byte aligned,
 *      sized by the totals); counters[AVDB_CTR_COPY_ROWS..HOST_LINES] accumulated.
 * line_state: AVDB_LINE_GPU rendered here; AVDB_LINE_HOST zero bytes — the host
 * renders the line (text the GPU does not canonicalise, or a line on which the
 * reference raises); AVDB_LINE_SKIP comment line ('#', load_vcf_file.py:103). */
#define AVDB_LINE_GPU 0
#define AVDB_LINE_HOST 1
#define AVDB_LINE_SKIP 2
#define AVDB_MAX_ALG_ID 64

#define AVDB_FORMAT_ADSP 1u           /* opts.flags: COPY rows end with is_adsp_variant = True
                                        * (vcf_variant_loader.py:336-337) */
typedef struct avdb_format_opts {
  uint32_t struct_size;   /* sizeof(avdb_format_opts) as the caller compiled it: the
                           * library refuses a size it does not know (ABI check) */
  uint32_t max_seq_len;   /* primary_key_generator.py:53 (default 50) */
  const char* alg_id;     /* xstr(row_algorithm_id), host NUL-terminated; NULL = "" */
  uint32_t flags;         /* AVDB_FORMAT_* */
  /* --skipExisting (optional, device; NULL = off): K6 match / kind per record and
   * the .mapping text each existing key contributes (its match list, rendered
   * once by the host): frag[frag_off[k] .. frag_off[k+1]).  A matched record gets
   * no COPY row, its fragment in the .mapping line, and counts as skipped
   * (vcf_variant_loader.py:285-291). */
  const int32_t* match;
  const uint8_t* match_kind;
  const uint8_t* frag;
  const uint64_t* frag_off;
  /* ADSP datasource (optional, device; NULL = off): per record, nonzero when its
   * primary key is already loaded (K6 avdb_keyset_probe_text over K7's keys):
   * is_duplicate(recordPK) -> an is_adsp_variant UPDATE instead of a COPY row, no
   * .mapping entry, counters[AVDB_CTR_ADSP_UPDATES] (vcf_variant_loader.py:303-307). */
  const uint8_t* adsp_dup;
} avdb_format_opts;

int avdb_format_workspace_size(size_t n, size_t* bytes);
int avdb_vcf_format_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                         const avdb_vcf_line* lines, const uint64_t* rec_off, const uint32_t* end,
                         const uint32_t* bin_code, const uint8_t* status, const char* digest,
                         const uint8_t* keep, const avdb_format_opts* opts, void* workspace,
                         size_t workspace_bytes, uint64_t* copy_off, uint64_t* map_off,
                         uint8_t* line_state, void* stream);
int avdb_vcf_format_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                          const avdb_vcf_line* lines, const uint64_t* rec_off, const uint32_t* end,
                          const uint32_t* bin_code, const uint8_t* status, const char* digest,
                          const uint8_t* keep, const avdb_format_opts* opts, const uint64_t* copy_off,
                          const uint64_t* map_off, const uint8_t* line_state, uint8_t* copy_out,
                          uint8_t* map_out, uint64_t* counters, void* stream);
/* K5h: ONE line of VCF text (host memory, no newline needed) -> its COPY rows and
 * .mapping line, rendered by the library's host code with the kernels' own
 * per-line definitions (K0 parse_line, K2 infer_end/classify, K5 format_line).
 * The per-line call of the reference's loader (VCFVariantLoader.parse_variant,
 * vcf_variant_loader.py:351-391, called per line by load_vcf_file.py:112) pays no
 * GPU launch + sync this way.  res->state: AVDB_LINE_GPU = rendered (the same
 * bytes the K5 kernels write for this line), AVDB_LINE_HOST = the caller renders
 * it (same rules as K5: non-canonical text, long alleles, unmappable records, ...),
 * AVDB_LINE_SKIP = comment.  opts: alg_id, max_seq_len, flags (AVDB_FORMAT_ADSP);
 * vcf_opts (nullable): header width and chromosome map as for avdb_vcf_parse_lines;
 * match / adsp_dup must be NULL (batch features).  Returns AVDB_ERANGE when a
 * buffer is short (res holds the sizes).  A context made with device = -1
 * suffices; thread-safe per calling thread. */
typedef struct avdb_line_result {
  uint32_t state;
  uint32_t flags;        /* K0 AVDB_VCF_* flags of the line */
  uint32_t copy_bytes;   /* COPY rows written (each ends with '\n') */
  uint32_t map_bytes;    /* .mapping line written: id '\t' [ {...}, ... ] '\n' */
  uint32_t n_rec;        /* records (ALT != '.') */
  uint32_t n_rows;       /* COPY rows */
  uint32_t n_skip;       /* ALT '.' skipped */
  uint32_t n_dup;
  uint32_t n_upd;
  uint32_t reserved;
} avdb_line_result;
int avdb_vcf_line_host(const avdb_ctx* ctx, const char* line, size_t len, const avdb_format_opts* opts,
                       const avdb_vcf_opts* vcf_opts, char* copy_out, size_t copy_cap, char* map_out,
                       size_t map_cap, avdb_line_result* res);
/* get_display_attributes (variant_annotator.py:134-241) of a record batch as
 * json.dumps text (ASCII alleles; json escaping applied).  end = K2's end.
 * Call with out == NULL first: rec_state[i] (0 ok, 1 non-ASCII allele, 2 heap
 * overrun) and exclusive offsets out_off[n+1]; then with out (8-byte aligned,
 * out_off[n] bytes).  Contigs >= 25 get no label inside normalized_metaseq_id. */
int avdb_display_attributes(avdb_ctx* ctx, const uint8_t* chrom, const uint32_t* pos, const uint32_t* end,
                            const uint64_t* allele_off, const uint32_t* ref_len, const uint32_t* alt_len,
                            const uint8_t* heap, size_t heap_bytes, size_t n, void* workspace,
                            size_t workspace_bytes, uint64_t* out_off, uint8_t* out, uint8_t* rec_state,
                            void* stream);

/* ---- K7: primary keys and bin paths of a record batch as text -----------
 * Replaces VariantPKGenerator.generate_primary_key (primary_key_generator.py:99-122,
 * the record_primary_key column) and the ltree text BinIndex.find_bin_index
 * returns (bin_index.py:75) for a whole record batch:
 *   key  = <contig label> ':' pos ':' ref ':' alt [':' 'rs'<ext_id>]   (short)
 *          <contig label> ':' pos ':' <digest>   [':' 'rs'<ext_id>]   (ref_len + alt_len
 *          > max_seq_len; digest = avdb_vrs_digest output, 32 chars per record)
 *   path = avdb_format_bin_path(chrom, bin_code) (bin_code NULL: no paths)
 * ext_id is rendered 'rs' + decimal (canonical refSNP keys, < 2^63).
 * Call with key_out == NULL first: exclusive offsets key_off[n+1] (and
 * path_off[n+1]) from the SoA alone; then with key_out (and path_out), 8-byte
 * aligned, of key_cap (path_cap) bytes >= the totals, which writes the text and
 * key_state[n] (a text that would end past its cap is not written, and its record's
 * state says so: AVDB_KEY_OVERFLOW / AVDB_PATH_OVERFLOW).  The write call runs the
 * one-pass write pass below (workspace: avdb_format_workspace_size(n) bytes, 16-byte
 * aligned) and writes the same key_off / path_off again: */
#define AVDB_KEY_OK 0
#define AVDB_KEY_HOST 1          /* ':' in an allele (the reference raises ValueError),
                                  * non-ASCII bytes, a contig without label or an
                                  * interned (non-rs) external id: caller renders */
#define AVDB_KEY_NEED_DIGEST 2   /* long record and digest == NULL */
#define AVDB_KEY_OVERFLOW 3      /* the key would end past key_cap: not written */
#define AVDB_KEY_DIGEST_PENDING 4 /* long record under AVDB_KEYS_DIGEST_DEFERRED: the key is
                                  * written except its 32 digest characters (zero bytes)
                                  * until avdb_primary_keys_fill_digests sets them and the
                                  * state to AVDB_KEY_OK */
#define AVDB_PATH_OVERFLOW 0x10u /* ORed in: the path would end past path_cap: not written */
int avdb_primary_keys(avdb_ctx* ctx, const uint8_t* chrom, const uint32_t* pos, const uint64_t* allele_off,
                      const uint32_t* ref_len, const uint32_t* alt_len, const uint8_t* heap,
                      size_t heap_bytes, const uint64_t* ext_id, const uint32_t* bin_code,
                      const char* digest, size_t n, uint32_t max_seq_len, void* workspace,
                      size_t workspace_bytes, uint64_t* key_off, uint64_t* path_off, uint8_t* key_out,
                      size_t key_cap, uint8_t* path_out, size_t path_cap, uint8_t* key_state,
                      void* stream);

/* K7 without a host round trip: per group of 64 / 256 records the key and path
 * byte totals (or the keyed K2's), one scan over the group totals, then the write
 * pass, which recomputes each record's sizes from the SoA it reads anyway, writes
 * the offsets and renders the text.  Same inputs and outputs as
 * avdb_primary_keys, except that key_off[n+1] / path_off[n+1] are OUTPUTS and the
 * text buffers are sized in advance: avdb_primary_keys_bound gives capacities no
 * batch of n records with heap_bytes of alleles can exceed.  workspace:
 * avdb_primary_keys_onepass_workspace_size(n) bytes, 8-byte aligned. */
int avdb_primary_keys_bound(size_t n, size_t heap_bytes, size_t* key_cap, size_t* path_cap);
int avdb_primary_keys_onepass_workspace_size(size_t n, size_t* bytes);
int avdb_primary_keys_onepass(avdb_ctx* ctx, const uint8_t* chrom, const uint32_t* pos, const uint64_t* allele_off,
                              const uint32_t* ref_len, const uint32_t* alt_len, const uint8_t* heap,
                              size_t heap_bytes, const uint64_t* ext_id, const uint32_t* bin_code,
                              const char* digest, size_t n, uint32_t max_seq_len, void* workspace,
                              size_t workspace_bytes, uint64_t* key_off, uint64_t* path_off, uint8_t* key_out,
                              size_t key_cap, uint8_t* path_out, size_t path_cap, uint8_t* key_state,
                              void* stream);
/* The same with flags: AVDB_KEYS_TOTALS_READY = the workspace already holds the
 * group totals avdb_record_prep_keyed wrote for this batch (same n, max_seq_len,
 * digest presence and paths), so the totals pass over the SoA is skipped (only
 * the last group is summed again, inside the scan). */
#define AVDB_KEYS_TOTALS_READY 1u
/* AVDB_KEYS_DIGEST_DEFERRED (digest == NULL): long records' keys are laid out with
 * their 32 digest characters still to come (state AVDB_KEY_DIGEST_PENDING), so K7
 * need not wait for K4: run avdb_vrs_digest beside it (another stream) and then
 * avdb_primary_keys_fill_digests.  The keyed K2 totals for this are the ones made
 * with has_digest != 0. */
#define AVDB_KEYS_DIGEST_DEFERRED 2u
/* AVDB_KEYS_OFF32: key_off / path_off in the narrow layout, each a buffer of
 * avdb_keys_off32_bytes(n) bytes (8-byte aligned): n + 1 uint32 low words (offset mod
 * 2^32), then from the next 8-byte boundary one uint64 base per 4,096 records (the
 * full offset of record 4096 k).  Full offset of i = base[i >> 12] +
 * (uint32_t)(low[i] - (uint32_t)base[i >> 12]) (4,096 records' text is < 4 GB).
 * 4 bytes per record and stream are written instead of 8.  Not accepted by
 * avdb_primary_keys_fill_digests / avdb_vrs_digest_keys / avdb_keyset_probe_text,
 * which take uint64 offsets. */
#define AVDB_KEYS_OFF32 4u
int avdb_keys_off32_bytes(size_t n, size_t* bytes);
int avdb_primary_keys_onepass_ex(avdb_ctx* ctx, const uint8_t* chrom, const uint32_t* pos,
                                 const uint64_t* allele_off, const uint32_t* ref_len, const uint32_t* alt_len,
                                 const uint8_t* heap, size_t heap_bytes, const uint64_t* ext_id,
                                 const uint32_t* bin_code, const char* digest, size_t n, uint32_t max_seq_len,
                                 void* workspace, size_t workspace_bytes, uint64_t* key_off, uint64_t* path_off,
                                 uint8_t* key_out, size_t key_cap, uint8_t* path_out, size_t path_cap,
                                 uint8_t* key_state, uint32_t flags, void* stream);
/* The digest characters of every AVDB_KEY_DIGEST_PENDING key: digest = the
 * avdb_vrs_digest output for the same batch (32 chars per record, 16-byte
 * aligned), key_off / key_out / key_state = the deferred K7 call's (key_state
 * 16-byte aligned).  Each pending key's state becomes AVDB_KEY_OK. */
int avdb_primary_keys_fill_digests(avdb_ctx* ctx, const uint8_t* chrom, const uint32_t* pos, size_t n,
                                   const char* digest, const uint64_t* key_off, uint8_t* key_out,
                                   uint8_t* key_state, void* stream);
/* K2 that also writes K7's group totals (key / path bytes per group of 64 or 256
 * records) into a one-pass K7 workspace, from the SoA it reads anyway plus the
 * refSNP ids: the record-prep half of the keyed pipeline (C4k, C1).  With a K4
 * workspace (avdb_vrs_digest_workspace_size(n) bytes, 16-byte aligned; nullable)
 * it also classifies every record for K4 (short, or long and its SHA-512 block
 * bucket).  With a K3 list workspace and a keep array (nullable) it also runs K3's
 * first phase (keep = 1; listed per workgroup: the records that share (chrom, pos)
 * with their predecessor and either have its ref / alt lengths and ext_id or are
 * third or later at their position — the others cannot repeat an earlier primary
 * key) when its lists fit (kDedupListHead + 4 * grid * slice bytes: at most
 * 16 KB + 4 (n + 2^22) at the default unroll).  The resolve (avdb_pk_dedup_ex with
 * AVDB_DEDUP_MARKED) must then be given the same ext_id.  key_workspace NULL: no
 * K7 totals (a step without key text, as C5's: K4's codes and K3's marks only).
 * *totals_written = AVDB_KEYED_TOTALS | AVDB_KEYED_LONG_CODES | AVDB_KEYED_DEDUP_MARKS
 * for what it wrote (16-byte aligned arrays; else 0 and it is avdb_record_prep):
 * pass AVDB_KEYS_TOTALS_READY to avdb_primary_keys_onepass_ex, AVDB_DIGEST_CODES_READY
 * to avdb_vrs_digest_ex (same n and max_seq_len) and AVDB_DEDUP_MARKED to
 * avdb_pk_dedup_ex then. */
#define AVDB_KEYED_TOTALS 1
#define AVDB_KEYED_LONG_CODES 2
#define AVDB_KEYED_DEDUP_MARKS 4
int avdb_record_prep_keyed(avdb_ctx* ctx, const uint8_t* chrom, const uint32_t* pos, const uint64_t* allele_off,
                           const uint32_t* ref_len, const uint32_t* alt_len, const uint8_t* heap, size_t heap_bytes,
                           size_t n, uint32_t* end_out, uint32_t* bin_code, uint8_t* status, uint32_t* lcp,
                           uint32_t* hist_l8, uint64_t* counters, const uint64_t* ext_id, uint32_t max_seq_len,
                           int has_digest, int with_paths, void* key_workspace, size_t key_workspace_bytes,
                           void* digest_workspace, size_t digest_workspace_bytes, void* dedup_workspace,
                           size_t dedup_workspace_bytes, uint8_t* keep, int* totals_written, void* stream);

/* The keyed step's record prep and text in ONE pass (round 6; the SoA read once):
 * what avdb_record_prep_keyed followed by avdb_primary_keys_onepass_ex compute —
 * end_out, bin_code, status (nullable); hist_l8 / counters accumulated (nullable); with
 * a K4 workspace (nullable) K4's long-record codes (then avdb_vrs_digest_ex with
 * AVDB_DIGEST_CODES_READY); with a K3 list workspace and keep (nullable) K3's first
 * phase (then avdb_pk_dedup_ex with AVDB_DEDUP_MARKED | AVDB_DEDUP_ONEPASS); and the
 * keys, ltree paths (path_out nullable: none), key_off[n+1] / path_off[n+1] and
 * key_state exactly as avdb_primary_keys_onepass_ex with digest == NULL (flags:
 * AVDB_KEYS_DIGEST_DEFERRED lays long keys out for avdb_primary_keys_fill_digests;
 * without it they are AVDB_KEY_NEED_DIGEST).  Text capacities as
 * avdb_primary_keys_bound.  workspace: avdb_keyed_prep_workspace_size(n) bytes,
 * 16-byte aligned (48 B per group of 1,024 records).  Groups of 256 records take their text
 * offsets from a decoupled look-back in the launch; *written = AVDB_KEYED_LONG_CODES |
 * AVDB_KEYED_DEDUP_MARKS for what it wrote.  avdb_keyed_prep_lookback_errors reads
 * (synchronously) how many look-back polls gave up in the last call on this workspace
 * (0 always expected; non-zero means its offsets are not valid). */
int avdb_keyed_prep_workspace_size(size_t n, size_t* bytes);
int avdb_keyed_prep(avdb_ctx* ctx, const uint8_t* chrom, const uint32_t* pos, const uint64_t* allele_off,
                    const uint32_t* ref_len, const uint32_t* alt_len, const uint8_t* heap, size_t heap_bytes,
                    const uint64_t* ext_id, size_t n, uint32_t max_seq_len, uint32_t* end_out, uint32_t* bin_code,
                    uint8_t* status, uint32_t* hist_l8, uint64_t* counters, void* workspace, size_t workspace_bytes,
                    void* digest_workspace, size_t digest_workspace_bytes, void* dedup_workspace,
                    size_t dedup_workspace_bytes, uint8_t* keep, uint64_t* key_off, uint64_t* path_off,
                    uint8_t* key_out, size_t key_cap, uint8_t* path_out, size_t path_cap, uint8_t* key_state,
                    uint32_t flags, int* written, void* stream);
int avdb_keyed_prep_lookback_errors(avdb_ctx* ctx, const void* workspace, uint32_t* out);

/* ---- K8: the per-record drop-in path in one launch -------------------------
 * The reference calls its per-record API once per alt allele
 * (vcf_variant_loader.py:282-311: __generate_primary_key, infer_variant_end_location,
 * find_bin_index, get_display_attributes).  For a small batch (one VCF line, one
 * find_bin_index miss) this entry does K2 + K7 + K5a in ONE launch of one
 * workgroup; every array may live in host-mapped pinned memory (avdb_host_alloc),
 * so a call is one launch + one stream sync, no copies.
 * Inputs: chrom, pos, and either end_in (bin of [pos, end_in]) or the alleles
 * (allele_off/ref_len/alt_len/heap, ext_id nullable: end inferred).  Outputs:
 * end_out, code, status per record; with alleles key_state (AVDB_KEY_*) and
 * disp_state (0 ok, 1 non-ASCII, 2 heap overrun); text streams selected by `want`
 * (AVDB_SMALL_PATH / _KEY / _DISPLAY) into text_out[k] (8-byte aligned, text_cap[k]
 * bytes) with offsets off_out[k*(n+1) + i] (u32).  A stream whose total exceeds
 * its cap is not written and sets bit k of *overflow. */
#define AVDB_SMALL_PATH 1u
#define AVDB_SMALL_KEY 2u
#define AVDB_SMALL_DISPLAY 4u
#define AVDB_SMALL_MAX 65536
typedef struct avdb_small_batch {
  const uint8_t* chrom;
  const uint32_t* pos;
  const uint32_t* end_in;
  const uint64_t* allele_off;
  const uint32_t* ref_len;
  const uint32_t* alt_len;
  const uint8_t* heap;
  const uint64_t* ext_id;
  size_t heap_bytes;
  uint32_t n;
  uint32_t max_seq_len;
  uint32_t want;
  uint32_t reserved;
  uint32_t* end_out;
  uint32_t* code;
  uint8_t* status;
  uint8_t* key_state;
  uint8_t* disp_state;
  uint32_t* off_out;
  uint8_t* text_out[3];
  uint32_t text_cap[3];
  uint32_t* overflow;
} avdb_small_batch;
int avdb_small_prep(avdb_ctx* ctx, const avdb_small_batch* batch, void* stream);
/* K8h: the same outputs computed by the library's host code from the kernels'
 * own record arithmetic (infer_end / classify / bin_path / display_json are
 * compiled for both sides), for callers that arrive one record or one VCF line
 * at a time — BinIndex.find_bin_index (bin_index.py:59-75) and
 * VCFVariantLoader.parse_variant (vcf_variant_loader.py:351-391) — where a GPU
 * launch + stream sync would cost more than the reference's whole call.  All
 * arrays are host memory; no stream, no device.  A context made with
 * device = -1 suffices. */
int avdb_small_prep_host(const avdb_ctx* ctx, const avdb_small_batch* batch);
/* K1h: the bin code, status and ltree path of ONE interval [start, end] (end >=
 * start; swapped intervals get status END_BEFORE_START as in K1) on the host —
 * one BinIndex.find_bin_index cache miss (bin_index.py:43-56,75).  Returns the
 * path length written to out (host, no NUL), 0 when unmappable (code ==
 * AVDB_BIN_NONE, or a contig beyond the labelled 25), or AVDB_ERANGE. */
int avdb_bin_path_host(const avdb_ctx* ctx, uint8_t chrom, uint32_t start, uint32_t end, uint32_t* code,
                       uint8_t* status, char* out_host, size_t cap);
/* K8a: ONE VariantAnnotator (Util/lib/python/variant_annotator.py:21-241) on the
 * host, for the drop-in class the reference constructs per alt allele
 * (vcf_parser.py:225-231, vcf_variant_loader.py:309-311).  alleles = REF bytes
 * then ALT bytes (host).  end_rel = infer_variant_end_location - pos (:36-79,
 * relative, so the caller's integer position is never narrowed); lcp = the
 * common-prefix length __normalize_alleles trims (:82-121).  With want_display,
 * the get_display_attributes fields (:134-241): location_start / _end, the class,
 * and the display_allele then sequence_allele texts in text[0, display_bytes +
 * sequence_bytes) — state 0; state 1 when they are the caller's (a non-ASCII
 * allele, or coordinates leaving u32), 2 when not asked.  Returns 0, or
 * AVDB_ERANGE when the two texts exceed cap (their sizes are set). */
#define AVDB_VC_SNV 0          /* single nucleotide variant / SNV */
#define AVDB_VC_INVERSION 1    /* inversion / MNV */
#define AVDB_VC_SUBSTITUTION 2 /* substitution / MNV */
#define AVDB_VC_INDEL 3        /* indel / INDEL */
#define AVDB_VC_INDEL_DOWN 4   /* indel / INDEL (insertion downstream of POS) */
#define AVDB_VC_INSERTION 5    /* insertion / INS */
#define AVDB_VC_DUPLICATION 6  /* duplication / DUP */
#define AVDB_VC_DELETION 7     /* deletion / DEL */
typedef struct avdb_annotation {
  int32_t end_rel;
  uint32_t lcp;
  uint32_t location_start;
  uint32_t location_end;
  uint32_t variant_class;
  uint32_t display_bytes;
  uint32_t sequence_bytes;
  uint32_t state;
} avdb_annotation;
int avdb_annotate_host(const avdb_ctx* ctx, const uint8_t* alleles, uint32_t ref_len, uint32_t alt_len,
                       uint32_t pos, int want_display, avdb_annotation* out, char* text, size_t cap);
/* Pinned host memory mapped into the device address space (hipHostMalloc,
 * mapped + coherent): the same pointer is valid on the host and in kernels. */
int avdb_host_alloc(size_t bytes, void** ptr);
int avdb_host_free(void* ptr);

/* ---- K6: duplicate check against variants already loaded ---------------
 * Replaces VariantRecord.exists / SQL map_variants(id, firstHitOnly, checkAltVariants)
 * (Util/lib/python/database/variant.py:41,287-309) as used by --skipExisting
 * (vcf_variant_loader.py:284-291).  The existing rows' metaseq ids form a key
 * set: keys = concatenated bytes, key_off[n_keys+1] (device).  build fills a
 * table of avdb_keyset_workspace_size(n_keys) bytes; probe writes per record
 * match[i] = index of the first equal key or -1, and kind[i]: */
#define AVDB_MATCH_NONE 0
#define AVDB_MATCH_EXACT 1              /* chrom:pos:ref:alt */
#define AVDB_MATCH_SWITCHED 2           /* chrom:pos:alt:ref (check_alt) */
#define AVDB_MATCH_HOST 255             /* contig without a canonical label: caller resolves */
int avdb_keyset_workspace_size(size_t n_keys, size_t* bytes);
int avdb_keyset_build(avdb_ctx* ctx, const uint8_t* keys, const uint64_t* key_off, size_t n_keys, void* table,
                      size_t table_bytes, void* stream);
/* the same table built on the host (host arrays): it answers every probe as avdb_keyset_build's
 * does, though not necessarily slot for slot */
int avdb_keyset_build_host(const avdb_ctx* ctx, const uint8_t* keys, const uint64_t* key_off, size_t n_keys,
                           void* table, size_t table_bytes);
int avdb_keyset_probe(avdb_ctx* ctx, const void* table, size_t table_bytes, const uint8_t* keys,
                      const uint64_t* key_off, size_t n_keys, const uint8_t* chrom, const uint32_t* pos,
                      const uint64_t* allele_off, const uint32_t* ref_len, const uint32_t* alt_len,
                      const uint8_t* heap, size_t heap_bytes, size_t n, int check_alt, int32_t* match,
                      uint8_t* kind, uint64_t* counters, void* stream);
/* The same key set probed with arbitrary strings q[q_off[i] .. q_off[i+1]) (device),
 * e.g. the primary keys avdb_primary_keys rendered: ADSP loads check each record's
 * primary key against the rows already loaded (is_duplicate(recordPK),
 * vcf_variant_loader.py:303-307).  match[i] = first equal key or -1; rows with
 * skip[i] != 0 (nullable) are not probed (-1). */
int avdb_keyset_probe_text(avdb_ctx* ctx, const void* table, size_t table_bytes, const uint8_t* keys,
                           const uint64_t* key_off, size_t n_keys, const uint8_t* q, const uint64_t* q_off,
                           const uint8_t* skip, size_t n, int32_t* match, uint64_t* counters, void* stream);

/* ---- K10: CADD score annotation -------------------------------------------
 * Replaces the per-variant tabix fetch of CADDUpdater.buffer_variant
 * (Util/lib/python/loaders/cadd_updater.py:175-221, driven by
 * Load/bin/load_cadd_scores.py) with a sort-merge join of a record batch against
 * a CADD table held on the device.
 * K10a, avdb_cadd_table_build: `text` is a slab of uncompressed CADD TSV ('#'
 * header lines, then Chrom<TAB>Pos<TAB>Ref<TAB>Alt<TAB>RawScore<TAB>PHRED[<TAB>...],
 * '\n'-separated, the last '\n' optional; n_lines as for K0: newlines + (text
 * does not end in '\n'), avdb_vcf_count_lines counts them).  One row per data
 * line (not empty, not '#'), in file order, into columns of n_lines entries each:
 *   chrom    contig code; CADD's MT is the project's M; 255 unknown (never matches
 *            on the device)
 *   pos      1-based position
 *   ref_off / ref_len / alt_off / alt_len   the alleles, as offsets into `text`
 *            itself (the table keeps the slab; nothing is copied)
 *   raw / phred   the scores: -?digits[.digits] of at most 15 significant and 22
 *            fractional digits is parsed on the device to the double Python's
 *            float() gives; any other text is flagged AVDB_CADD_ROW_SCORE_HOST and
 *            left 0.0 for the caller to parse
 *   flags    AVDB_CADD_ROW_*; a row with fewer than 6 fields or a POS that is not
 *            a plain decimal in [1, 2^32) is AVDB_CADD_ROW_BAD and never matches
 *            (chrom 255, both allele offsets the line's own, lengths and scores 0;
 *            pos: that of the nearest earlier row that is not BAD when at most 64
 *            BAD rows lie between, else 0)
 * first_row[c] / end_row[c] (u32[AVDB_CADD_N_CONTIGS]): the rows of contig c
 * (first_row >= end_row: none).  counts (device, 4 x u64): AVDB_CADD_COUNT_*;
 * an order violation is a contig whose rows are not one contiguous run, a pos
 * that decreases inside a run, or more than 64 AVDB_CADD_ROW_BAD rows in a row —
 * the order tabix requires; a table with violations must not be joined against.
 * Workspace: avdb_cadd_workspace_size bytes, 256-byte aligned.
 * K10b, avdb_cadd_match: per record (the arrays avdb_keyset_probe takes) the
 * indel table is searched when ref_len > 1 or alt_len > 1, the SNV table
 * otherwise (either may be NULL or empty); among the rows at the record's
 * position the first, in file order, with
 *   (ref == R || ref == A) && (alt == R || alt == A)     (R, A: the row's alleles)
 * is the answer, exactly the reference's test (cadd_updater.py:202-204: a
 * switched row matches).  row[i] = its index or -1; kind[i] = AVDB_CADD_*;
 * raw[i] / phred[i] are written for matched records only.  counters (nullable,
 * device, 3 x u64, added to): AVDB_CADD_CTR_*.
 * The _host entries run the same per-line and per-record code in a loop on host
 * memory, with a context from avdb_ctx_create(-1, ...). */
#define AVDB_CADD_N_CONTIGS 25
#define AVDB_CADD_ROW_SCORE_HOST 0x01u  /* a score the device does not parse: caller's float() */
#define AVDB_CADD_ROW_BAD 0x02u         /* < 6 fields or POS not a plain decimal in [1, 2^32) */
#define AVDB_CADD_NONE 0
#define AVDB_CADD_SNV 1                 /* matched in the SNV table */
#define AVDB_CADD_INDEL 2               /* matched in the indel table */
#define AVDB_CADD_HOST 255              /* record contig 255: the caller resolves it by name */
#define AVDB_CADD_COUNT_ROWS 0
#define AVDB_CADD_COUNT_SCORE_HOST 1
#define AVDB_CADD_COUNT_BAD 2
#define AVDB_CADD_COUNT_ORDER_VIOLATIONS 3
#define AVDB_CADD_N_COUNTS 4
#define AVDB_CADD_CTR_SNV 0
#define AVDB_CADD_CTR_INDEL 1
#define AVDB_CADD_CTR_NOT_MATCHED 2
#define AVDB_CADD_N_CTRS 3
typedef struct avdb_cadd_table {
  uint32_t struct_size;     /* sizeof(avdb_cadd_table) */
  uint32_t reserved;
  uint64_t n_rows;          /* 0: an empty table (the pointers are not read) */
  const uint8_t* text;      /* the slab the table was built from */
  uint64_t text_bytes;
  const uint8_t* chrom;
  const uint32_t* pos;
  const uint64_t* ref_off;
  const uint32_t* ref_len;
  const uint64_t* alt_off;
  const uint32_t* alt_len;
  const double* raw;
  const double* phred;
  const uint8_t* flags;
  const uint32_t* first_row;
  const uint32_t* end_row;
} avdb_cadd_table;
int avdb_cadd_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes);
int avdb_cadd_table_build(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, uint8_t* chrom,
                          uint32_t* pos, uint64_t* ref_off, uint32_t* ref_len, uint64_t* alt_off, uint32_t* alt_len,
                          double* raw, double* phred, uint8_t* flags, uint32_t* first_row, uint32_t* end_row,
                          uint64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int avdb_cadd_match(avdb_ctx* ctx, const avdb_cadd_table* snv, const avdb_cadd_table* indel, const uint8_t* chrom,
                    const uint32_t* pos, const uint64_t* allele_off, const uint32_t* ref_len, const uint32_t* alt_len,
                    const uint8_t* heap, size_t heap_bytes, size_t n, int32_t* row, uint8_t* kind, double* raw,
                    double* phred, uint64_t* counters, void* stream);
int avdb_cadd_table_build_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                               uint8_t* chrom, uint32_t* pos, uint64_t* ref_off, uint32_t* ref_len, uint64_t* alt_off,
                               uint32_t* alt_len, double* raw, double* phred, uint8_t* flags, uint32_t* first_row,
                               uint32_t* end_row, uint64_t* counts);
int avdb_cadd_match_host(const avdb_ctx* ctx, const avdb_cadd_table* snv, const avdb_cadd_table* indel,
                         const uint8_t* chrom, const uint32_t* pos, const uint64_t* allele_off,
                         const uint32_t* ref_len, const uint32_t* alt_len, const uint8_t* heap, size_t heap_bytes,
                         size_t n, int32_t* row, uint8_t* kind, double* raw, double* phred, uint64_t* counters);

/* ---- K11: BGZF (bgzip) input inflated on the GPU ------------------------------
 * The files the reference loads arrive as bgzip (.vcf.gz, CADD's .tsv.gz with a .tbi):
 * a chain of independent gzip members (SAM specification 4.1), each of at most 64 KiB
 * of output, each stating its compressed size (BSIZE in the 'BC' extra subfield) and
 * its output size (ISIZE in the trailer).
 *
 * avdb_bgzf_index_host walks the members of data[0 .. bytes) (host memory).  A member
 * carries magic 1f 8b, CM 8, FLG 4 (FEXTRA), a 'BC' subfield of length 2 (other extra
 * subfields before or after it are skipped), BSIZE + 1 >= its header and trailer, and
 * ISIZE <= 65536.  in_off[k] (blocks_cap entries) is the offset of member k, out_off[k]
 * (blocks_cap + 1 entries) the exclusive sum of ISIZE, out_off[*n_blocks] = *out_bytes;
 * *consumed is the offset after the last complete member.  The walk stops without error
 * at a member that runs past `bytes` (a caller streaming a file carries the tail over)
 * and after blocks_cap members (call again from *consumed).  AVDB_ENOTBGZF: the first
 * member is gzip (magic, CM 8) but no BGZF member; AVDB_EINVAL: no gzip magic there, or
 * a malformed member later in the chain (avdb_last_error names its offset).
 *
 * avdb_bgzf_inflate (device pointers; avdb_bgzf_inflate_host: the same per-member code
 * on host pointers, on an avdb_ctx_create(-1, ...) context) writes member k's bytes to
 * out[out_off[k] .. out_off[k+1]) and its AVDB_BGZF_* code to status[k] (n_blocks
 * entries; out_off has n_blocks + 1).  Full RFC 1951 (stored, fixed and dynamic blocks,
 * any number per member), code sets accepted as zlib's inflate_table accepts them
 * (over-subscribed: refused; incomplete: refused unless a single code of length 1;
 * no end-of-block code, more than 286 literal/length or 30 distance codes: refused),
 * and the CRC-32 of the output checked against the trailer.  For any input bytes the
 * decoder reads only comp[0 .. comp_bytes) (a member: only its own extent) and writes
 * only the ranges of members whose status is AVDB_BGZF_OK: a member that fails writes
 * nothing.  counts[AVDB_BGZF_N_COUNTS] (set by the call): members OK, members failed,
 * index of the first failed member (~0 when none).  The device entry decodes each member
 * in a 64 KiB window of a workspace the context owns (allocated at the first call, one
 * window per workgroup of the grid, freed by avdb_ctx_destroy). */
#define AVDB_BGZF_OK 0
#define AVDB_BGZF_BAD_HEADER 1  /* no BGZF member at in_off[k], ISIZE != out_off[k+1] - out_off[k], a range outside
                                   comp / out, or a deflate stream that ends before the trailer */
#define AVDB_BGZF_OVERRUN 2     /* the deflate stream runs past the member's compressed extent */
#define AVDB_BGZF_BAD_BTYPE 3   /* block type 3 */
#define AVDB_BGZF_BAD_STORED 4  /* stored block: LEN != ~NLEN */
#define AVDB_BGZF_BAD_LENS 5    /* a code-length set zlib refuses */
#define AVDB_BGZF_BAD_SYMBOL 6  /* bits that are no code of the set, or literal/length 286-287, distance 30-31 */
#define AVDB_BGZF_DIST_FAR 7    /* a distance before the member's first byte */
#define AVDB_BGZF_OUT_LONG 8    /* more output than ISIZE */
#define AVDB_BGZF_OUT_SHORT 9   /* less output than ISIZE */
#define AVDB_BGZF_BAD_CRC 10    /* CRC-32 of the output != the trailer's */
#define AVDB_BGZF_COUNT_OK 0
#define AVDB_BGZF_COUNT_FAILED 1
#define AVDB_BGZF_COUNT_FIRST_FAILED 2
#define AVDB_BGZF_N_COUNTS 3
int avdb_bgzf_index_host(const uint8_t* data, size_t bytes, size_t blocks_cap, uint64_t* in_off, uint64_t* out_off,
                         size_t* n_blocks, size_t* consumed, uint64_t* out_bytes);
int avdb_bgzf_inflate(avdb_ctx* ctx, const uint8_t* comp, size_t comp_bytes, const uint64_t* in_off,
                      const uint64_t* out_off, size_t n_blocks, uint8_t* out, size_t out_cap, uint8_t* status,
                      uint64_t* counts, void* stream);
int avdb_bgzf_inflate_host(const avdb_ctx* ctx, const uint8_t* comp, size_t comp_bytes, const uint64_t* in_off,
                           const uint64_t* out_off, size_t n_blocks, uint8_t* out, size_t out_cap, uint8_t* status,
                           uint64_t* counts);

/* ---- K12: the --skipExisting key set from an export ------------------------------
 * Replaces the per-row host loop that turns an export of AnnotatedVDB.Variant,
 * `metaseq_id<TAB>record_primary_key<TAB>bin_index[<TAB>...]` lines separated by '\n',
 * into what K6 and K5 take: the key blob avdb_keyset_build hashes, the primary-key
 * blob avdb_keyset_probe_text's table is built over, and avdb_format_opts.frag /
 * frag_off.  `text` is a slab of the export; n_lines its line count (newlines, plus one
 * when the text does not end in one), as for K0 and K10a.
 * Row rule: one trailing '\r' before the '\n' is stripped; a line with fewer than 3
 * tab-separated fields, or whose first field is exactly `metaseq_id`, is skipped;
 * every other line is a row, in file order; fields after the third are ignored and
 * empty fields allowed.  A '\r' no '\n' follows is not a line end here (it is one for
 * Python's text mode): such bytes are counted in counts[AVDB_EXIST_COUNT_LONE_CR] and
 * the caller decides.  contig_mask: bit c for the canonical contig label c (1..22, X,
 * Y, M), bit 31 for every other label; the label is the text before the first ':' of
 * the metaseq id; a row whose bit is clear is skipped as if its line were absent
 * (AVDB_EXIST_ALL_CONTIGS keeps everything).
 *   1. avdb_existing_size : per row (n_lines entries allocated, rows written)
 *      key_len, pk_len, frag_len, flags and row_off (u64: the offset of the row's line
 *      in the slab; its pk field starts key_len + 1 bytes on), and counts (8 x u64,
 *      set by the call).
 *      frag_len is the length of {'primary_key': '<pk>', 'bin_index': '<bin>'}, the
 *      repr of the row's one-entry match list.  AVDB_EXIST_FRAG_HOST: the pk or bin
 *      field holds a byte outside 0x20..0x7E, a ' or a \, which repr does not render
 *      verbatim: the caller renders that fragment, and stores its length in
 *      frag_len[row] before the write pass.  AVDB_EXIST_NONCANON: the contig label is
 *      not one of the 25.
 *   2. avdb_existing_write (n_rows = counts[AVDB_EXIST_COUNT_ROWS]; the same text and
 *      n_lines, and the arrays the size pass wrote):
 *      scans the three length arrays into key_off / pk_off / frag_off (n_rows + 1
 *      entries each) and writes the blobs (8-byte aligned, caps in bytes).  The
 *      fragment span of a FRAG_HOST row is left unwritten.  totals (4 x u64): the three
 *      blob sizes and the number of blobs larger than their cap.  Nothing outside
 *      [0, total) of a blob is written, and nothing at all when a cap is too small:
 *      the host entry returns AVDB_ERANGE then; the device entry, which does not wait
 *      for its own scan, returns AVDB_OK and leaves totals[3] != 0 for the caller to
 *      read after the stream.  Lengths or row offsets that do not
 *      describe the text read as zero bytes, never outside the slab.
 * Workspace: avdb_existing_workspace_size bytes, 256-byte aligned; the device entries
 * allocate nothing per call.  The _host entries run the same per-line code on host
 * pointers, on an avdb_ctx_create(-1, ...) context. */
#define AVDB_EXIST_FRAG_HOST 0x01u
#define AVDB_EXIST_NONCANON 0x02u
#define AVDB_EXIST_ALL_CONTIGS 0xFFFFFFFFu
#define AVDB_EXIST_COUNT_ROWS 0
#define AVDB_EXIST_COUNT_SKIPPED 1      /* lines that are no row */
#define AVDB_EXIST_COUNT_FRAG_HOST 2
#define AVDB_EXIST_COUNT_NONCANON 3
#define AVDB_EXIST_COUNT_LONE_CR 4
#define AVDB_EXIST_COUNT_KEY_BYTES 5    /* blob totals with the size pass's own frag_len */
#define AVDB_EXIST_COUNT_PK_BYTES 6
#define AVDB_EXIST_COUNT_FRAG_BYTES 7
#define AVDB_EXIST_N_COUNTS 8
int avdb_existing_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes);
int avdb_existing_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, uint32_t contig_mask,
                       uint32_t* key_len, uint32_t* pk_len, uint32_t* frag_len, uint8_t* flags, uint64_t* row_off, uint64_t* counts,
                       void* workspace, size_t workspace_bytes, void* stream);
int avdb_existing_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_rows,
                        const uint32_t* key_len, const uint32_t* pk_len, const uint32_t* frag_len,
                        const uint8_t* flags, const uint64_t* row_off, uint8_t* keys, size_t keys_cap,
                        uint64_t* key_off, uint8_t* pks, size_t pks_cap, uint64_t* pk_off, uint8_t* frag,
                        size_t frag_cap, uint64_t* frag_off, uint64_t* totals, void* workspace,
                        size_t workspace_bytes, void* stream);
int avdb_existing_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                            uint32_t contig_mask, uint32_t* key_len, uint32_t* pk_len, uint32_t* frag_len,
                            uint8_t* flags, uint64_t* row_off, uint64_t* counts);
int avdb_existing_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                             size_t n_rows, const uint32_t* key_len, const uint32_t* pk_len,
                             const uint32_t* frag_len, const uint8_t* flags, const uint64_t* row_off, uint8_t* keys,
                             size_t keys_cap, uint64_t* key_off, uint8_t* pks, size_t pks_cap, uint64_t* pk_off,
                             uint8_t* frag, size_t frag_cap, uint64_t* frag_off, uint64_t* totals);

/* ---- K13: CADD update rows from a variant export --------------------------------
 * Replaces the per-record host code around the K10 join in the CADD pass
 * (Load/bin/load_cadd_scores.py:109-120, cadd_updater.py:121-130,187-221): `text` is a
 * slab of an export in the column order of the reference's SELECT_SQL,
 * `record_primary_key<TAB>metaseq_id<TAB>cadd_scores[<TAB>...]` lines separated by '\n'
 * (n_lines as for K0, K10a and K12), and the output is the text of the update tuples,
 * one `pk<TAB>chrom<TAB>json<LF>` row per record that is not skipped.
 * Row rule: one trailing '\r' before the '\n' is stripped; an empty line, a line with
 * fewer than two fields and a line whose first field is exactly `record_primary_key`
 * are no row (counts[AVDB_CADDUPD_COUNT_SKIPPED_LINES]); fields after the third are
 * ignored.  A '\r' no '\n' follows is counted (AVDB_CADDUPD_COUNT_LONE_CR) and the
 * caller decides.  contig_mask: as for K12, over the label of the metaseq id (the text
 * before its first ':'); a line whose bit is clear is skipped as if it were absent.
 * With AVDB_CADDUPD_SKIP_EXISTING a line whose third field is present and neither empty
 * nor `\N` is counted in AVDB_CADDUPD_COUNT_SKIPPED and is no row.  Every other line is
 * a row, in file order:
 *   - a metaseq id without exactly three ':' is flagged AVDB_CADDUPD_BAD (no output);
 *   - label: 1..22, X, Y, M, and MT as M; position: 1 to 10 decimal digits below 2^32;
 *     the indel table when len(ref) > 1 or len(alt) > 1, else the SNV table; the K10
 *     join (avdb_cadd_match's row test) with the alleles read in the export text;
 *   - pk is copied verbatim; chrom is the caller's `chrom` text when chrom_len > 0
 *     (at most AVDB_CADDUPD_CHROM_MAX bytes, host memory), else `chr` + the bytes of
 *     pk before its first ':'; json is `{}` when no row matches, else
 *     `{"CADD_raw_score": R, "CADD_phred": P}` with R and P rewritten from the table's
 *     own score text into what Python's json.dumps(float(text)) gives (exact for every
 *     text K10a parses: the digits are kept, only zeros, the point and the exponent
 *     move);
 *   - a label outside the 25, a position that is not plain digits below 2^32, or a
 *     matched table row flagged AVDB_CADD_ROW_SCORE_HOST: AVDB_CADDUPD_ROW_HOST, output
 *     length 0; the caller renders the row, stores its length in out_len[row] before
 *     the write pass, and overwrites the row's span (filled with spaces) after it.
 *   1. avdb_cadd_update_size: per row (n_lines entries allocated, rows written)
 *      row_start (u64: the offset of the row's line in the slab), pk_len, kind
 *      (AVDB_CADD_NONE / _SNV / _INDEL), match (the table row, -1: none), out_len and
 *      row_flags; counts (AVDB_CADDUPD_N_COUNTS x u64, set by the call).  snv / indel /
 *      not_matched count the rows the device decided; out_bytes sums out_len.
 *   2. avdb_cadd_update_write (n_rows = counts[AVDB_CADDUPD_COUNT_ROWS]; the same text,
 *      tables, chrom and arrays): scans out_len into row_off (n_rows + 1 entries) and
 *      writes the rows to out (8-byte aligned, out_cap bytes).  totals (2 x u64): the
 *      bytes of all rows, and 1 when they exceed out_cap.  Nothing outside [0, total)
 *      is written, and nothing at all when out_cap is too small: the host entry returns
 *      AVDB_ERANGE then; the device entry, which does not wait for its own scan, returns
 *      AVDB_OK and leaves totals[1] != 0 for the caller to read after the stream.
 * avdb_cadd_score_text_host: the rewrite of one score text alone (out: cap >=
 * AVDB_CADDUPD_SCORE_MAX bytes); returns 1 and *len, or 0 for a text K10a leaves to the
 * host (AVDB_CADD_ROW_SCORE_HOST).
 * Workspace: avdb_cadd_update_workspace_size bytes, 256-byte aligned; the device entries
 * allocate nothing per call.  The _host entries run the same per-line code on host
 * pointers, on an avdb_ctx_create(-1, ...) context. */
#define AVDB_CADDUPD_ROW_HOST 0x01u
#define AVDB_CADDUPD_BAD 0x02u
#define AVDB_CADDUPD_SKIP_EXISTING 0x01u  /* avdb_cadd_update_size's flags */
#define AVDB_CADDUPD_CHROM_MAX 64
#define AVDB_CADDUPD_SCORE_MAX 24
#define AVDB_CADDUPD_COUNT_ROWS 0
#define AVDB_CADDUPD_COUNT_SKIPPED_LINES 1  /* lines that are no row and no skipped record */
#define AVDB_CADDUPD_COUNT_SKIPPED 2        /* records annotated already */
#define AVDB_CADDUPD_COUNT_SNV 3
#define AVDB_CADDUPD_COUNT_INDEL 4
#define AVDB_CADDUPD_COUNT_NOT_MATCHED 5
#define AVDB_CADDUPD_COUNT_HOST_ROWS 6
#define AVDB_CADDUPD_COUNT_BAD 7
#define AVDB_CADDUPD_COUNT_LONE_CR 8
#define AVDB_CADDUPD_COUNT_OUT_BYTES 9
#define AVDB_CADDUPD_N_COUNTS 10
int avdb_cadd_update_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes);
int avdb_cadd_update_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                          const avdb_cadd_table* snv, const avdb_cadd_table* indel, const char* chrom, size_t chrom_len,
                          uint32_t contig_mask, uint32_t flags, uint64_t* row_start, uint32_t* pk_len, uint8_t* kind,
                          int32_t* match, uint32_t* out_len, uint8_t* row_flags, uint64_t* counts, void* workspace,
                          size_t workspace_bytes, void* stream);
int avdb_cadd_update_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_rows,
                           const avdb_cadd_table* snv, const avdb_cadd_table* indel, const char* chrom,
                           size_t chrom_len, const uint64_t* row_start, const uint32_t* pk_len, const uint8_t* kind,
                           const int32_t* match, const uint32_t* out_len, const uint8_t* row_flags, uint8_t* out,
                           size_t out_cap, uint64_t* row_off, uint64_t* totals, void* workspace,
                           size_t workspace_bytes, void* stream);
int avdb_cadd_update_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                               const avdb_cadd_table* snv, const avdb_cadd_table* indel, const char* chrom,
                               size_t chrom_len, uint32_t contig_mask, uint32_t flags, uint64_t* row_start,
                               uint32_t* pk_len, uint8_t* kind, int32_t* match, uint32_t* out_len, uint8_t* row_flags,
                               uint64_t* counts);
int avdb_cadd_update_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                size_t n_rows, const avdb_cadd_table* snv, const avdb_cadd_table* indel,
                                const char* chrom, size_t chrom_len, const uint64_t* row_start, const uint32_t* pk_len,
                                const uint8_t* kind, const int32_t* match, const uint32_t* out_len,
                                const uint8_t* row_flags, uint8_t* out, size_t out_cap, uint64_t* row_off,
                                uint64_t* totals);
int avdb_cadd_score_text_host(const uint8_t* text, size_t n, uint8_t* out, size_t cap, size_t* len);

/* ---- K14: the per-chromosome VCF files of a variant export ----------------------
 * Replaces the per-record host code of Util/bin/export_variant2vcf.py (run, :63-97, and
 * print_file, :29-35): `text` is a slab of an export in the column order of the
 * reference's SELECT_SQL (:23),
 * `record_primary_key<TAB>metaseq_id<TAB>row_algorithm_id[<TAB>...]` lines separated by
 * '\n' (n_lines as for K0, K10a, K12 and K13), and the output is two texts: the rows of
 * the chrN_<k>.vcf files, in file order and without their header lines, and the rows of
 * chrN_invalid.txt.
 * Row rule (K13's): one trailing '\r' before the '\n' is stripped; an empty line, a line
 * with fewer than two fields and a line whose first field is exactly
 * `record_primary_key` are no row (counts[AVDB_EXPVCF_COUNT_SKIPPED_LINES]); fields after
 * the third are ignored.  A '\r' no '\n' follows is counted (AVDB_EXPVCF_COUNT_LONE_CR)
 * and the caller decides.  contig_mask: as for K12 and K13, over the label of the metaseq
 * id (the text before its first ':'); a line whose bit is clear is skipped as if it were
 * absent (AVDB_EXPVCF_COUNT_FILTERED).  Every other line is a row of one of two lists,
 * each in file order:
 *   - invalid: the metaseq id holds one of the bytes I, R, D, N anywhere (the
 *     reference's matches('I|R|D|N', metaseqId), taken as re.search; tested before
 *     anything else of the id).  Its text is `pk<TAB>alg<LF>`; alg is the third field
 *     verbatim, or `None` (how Python prints NULL) when that field is absent, empty or
 *     `\N`.  The reference reads a cursor, not text: that these three spell NULL is this
 *     project's choice, the one K13 makes for cadd_scores.
 *   - valid: every other row.  Its text is
 *     `label<TAB>pos<TAB>pk<TAB>ref<TAB>alt<TAB>.<TAB>.<TAB>.<LF>`, len(metaseq_id) +
 *     len(pk) + 8 bytes; the key and the four parts of the id are copied verbatim
 *     (backslashes too).  A valid row whose id does not have exactly three ':' is
 *     flagged AVDB_EXPVCF_BAD (no output; the reference's four-way unpack raises there).
 *     pk_hash: K6's 64-bit string hash of the key bytes, for the caller's search for
 *     repeated keys (the reference keeps a file's rows in a dict keyed by primary key).
 * Valid row v (BAD rows counted) belongs to file v / variants_per_file + 1, so the VCF
 * text of file k starts at row_off[(k - 1) * variants_per_file]; the split and the header
 * lines are the caller's.
 *   1. avdb_export_vcf_size: per valid row (n_lines entries allocated, rows written)
 *      row_start (u64: the offset of the row's line in the slab), pk_len, ms_len,
 *      out_len, row_flags, pk_hash; per invalid row inv_start, inv_pk_len, inv_out_len;
 *      counts (AVDB_EXPVCF_N_COUNTS x u64, set by the call).
 *   2. avdb_export_vcf_write, once per stream (`which`: AVDB_EXPVCF_STREAM_VCF with the
 *      valid rows' arrays, AVDB_EXPVCF_STREAM_INVALID with the invalid rows' and ms_len =
 *      row_flags = NULL; the same text): scans out_len into row_off (n_rows + 1 entries)
 *      and writes the rows to out (8-byte aligned, out_cap bytes).  Before it the caller
 *      may flag a valid row AVDB_EXPVCF_ROW_HOST and store the row's length in out_len
 *      (the row's span is filled with spaces, for the caller to overwrite after the
 *      pass), or AVDB_EXPVCF_DROPPED and store 0 (nothing is written for the row).
 *      totals (2 x u64): the bytes of all rows, and 1 when they exceed out_cap.  Nothing
 *      outside [0, total) is written, and nothing at all when out_cap is too small: the
 *      host entry returns AVDB_ERANGE then; the device entry, which does not wait for its
 *      own scan, returns AVDB_OK and leaves totals[1] != 0 for the caller to read after
 *      the stream.
 * Workspace: avdb_export_vcf_workspace_size bytes, 256-byte aligned; the device entries
 * allocate nothing per call.  The _host entries run the same per-line code on host
 * pointers, on an avdb_ctx_create(-1, ...) context. */
#define AVDB_EXPVCF_ROW_HOST 0x01u
#define AVDB_EXPVCF_BAD 0x02u
#define AVDB_EXPVCF_DROPPED 0x04u
#define AVDB_EXPVCF_STREAM_VCF 0u
#define AVDB_EXPVCF_STREAM_INVALID 1u
#define AVDB_EXPVCF_COUNT_VALID 0          /* BAD rows included */
#define AVDB_EXPVCF_COUNT_INVALID 1
#define AVDB_EXPVCF_COUNT_SKIPPED_LINES 2  /* lines that are no row and not filtered */
#define AVDB_EXPVCF_COUNT_FILTERED 3       /* lines of contigs outside contig_mask */
#define AVDB_EXPVCF_COUNT_BAD 4
#define AVDB_EXPVCF_COUNT_LONE_CR 5
#define AVDB_EXPVCF_COUNT_VCF_BYTES 6
#define AVDB_EXPVCF_COUNT_INVALID_BYTES 7
#define AVDB_EXPVCF_N_COUNTS 8
int avdb_export_vcf_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes);
int avdb_export_vcf_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, uint32_t contig_mask,
                         uint64_t* row_start, uint32_t* pk_len, uint32_t* ms_len, uint32_t* out_len,
                         uint8_t* row_flags, uint64_t* pk_hash, uint64_t* inv_start, uint32_t* inv_pk_len,
                         uint32_t* inv_out_len, uint64_t* counts, void* workspace, size_t workspace_bytes,
                         void* stream);
int avdb_export_vcf_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, uint32_t which,
                          size_t n_rows, const uint64_t* row_start, const uint32_t* pk_len, const uint32_t* ms_len,
                          const uint32_t* out_len, const uint8_t* row_flags, uint8_t* out, size_t out_cap,
                          uint64_t* row_off, uint64_t* totals, void* workspace, size_t workspace_bytes, void* stream);
int avdb_export_vcf_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                              uint32_t contig_mask, uint64_t* row_start, uint32_t* pk_len, uint32_t* ms_len,
                              uint32_t* out_len, uint8_t* row_flags, uint64_t* pk_hash, uint64_t* inv_start,
                              uint32_t* inv_pk_len, uint32_t* inv_out_len, uint64_t* counts);
int avdb_export_vcf_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                               uint32_t which, size_t n_rows, const uint64_t* row_start, const uint32_t* pk_len,
                               const uint32_t* ms_len, const uint32_t* out_len, const uint8_t* row_flags, uint8_t* out,
                               size_t out_cap, uint64_t* row_off, uint64_t* totals);

/* ---- K15: a whole-genome VCF split into per-chromosome texts ---------------------
 * Replaces the per-line host code of Util/bin/split_vcf_by_chr.py (run, :29-52): `text`
 * is a '\n'-separated slab of a VCF (n_lines as for K0, K10a and K12-K14) and the output
 * is one blob of 26 streams back to back: the data lines of chr1.vcf ... chr22.vcf,
 * chrX.vcf, chrY.vcf, chrM.vcf (streams 0..24, the order of the HumanChromosome enum) and
 * the lines the reference cannot place (stream AVDB_SPLIT_OTHER).  Inside a stream the
 * lines are in file order, each its stored bytes and a '\n'.  Header lines are the
 * caller's to write.
 * Line rule: a line's stored length is its length after Python's str.rstrip().  The
 * passes strip the six ASCII whitespace bytes (space, \t, \n, \v, \f, \r).  A line whose
 * last byte after that strip is 0x1C..0x1F or >= 0x80 is flagged AVDB_SPLIT_LINE_HOST,
 * bit 31 of its out_len, comments included: Python strips 0x1C..0x1F too, and the bytes
 * >= 0x80 may end a character it strips (U+0085, U+00A0, ...) or one its decode raises
 * on.  The caller decides such a line and stores its code and its out_len (the bit
 * cleared) before the write pass; Python's result is always a prefix of the line, so the
 * write pass needs nothing else.  The write pass ignores the bit.
 * A line whose first byte is '#' is a comment: no output, code AVDB_SPLIT_NONE, out_len
 * 0.  Every other line, the empty one too, has a key: its bytes before the first '\t',
 * or all of them.  Without a chromosome map the line's stream is c when the key is
 * exactly the c-th of the labels 1..22, X, Y, M (`chr1`, `MT`, `01`, `x`, `1 ` and the
 * empty key are none: the reference raises KeyError there).  With a map the key is
 * looked up as bytes and the stream is the key's code when that is below 25.  Every
 * other line goes to stream AVDB_SPLIT_OTHER, and counts[AVDB_SPLIT_COUNT_FIRST_OTHER] is
 * the smallest index of such a line (~0: none).
 * Invalid UTF-8 that does not sit at the stripped end of a line is copied verbatim,
 * where the reference's decode raises UnicodeDecodeError.
 *   1. avdb_vcf_split_size: per line code (u8), line_start (u64: the line's offset in
 *      the slab; an entry of a line past the text's own count is ~0) and out_len (u32:
 *      the stored length plus 1, 0 for a comment; bit 31: AVDB_SPLIT_LINE_HOST);
 *      counts (AVDB_SPLIT_N_COUNTS x u64, set by the call): the lines of each stream,
 *      the bytes of each stream, the comments, the LINE_HOST lines, first_other.
 *   2. avdb_vcf_split_write: the destination of every line (the exclusive sum of the
 *      out_len of the lines before it in its stream, after the streams before it) and
 *      the copy.  stream_off (27 x u64): the start of each stream in out and, in
 *      stream_off[26], the total.  dst_off (n_lines x u64, or NULL): each line's
 *      destination, ~0 for a line without output.  A code that is none of 0..25 gives no
 *      output.  totals (2 x u64): the bytes of all streams, and 1 when they exceed
 *      out_cap.  Nothing outside [0, total) is written, and nothing at all when out_cap
 *      is too small: the host entry returns AVDB_ERANGE then; the device entry, which
 *      does not wait for its own scan, returns AVDB_OK and leaves totals[1] != 0.
 * Workspace: avdb_vcf_split_workspace_size bytes, 256-byte aligned; the device entries
 * allocate nothing per call.  The _host entries run the same per-line code on host
 * pointers, on an avdb_ctx_create(-1, ...) context (chrom_map made on that context). */
#define AVDB_SPLIT_N_STREAMS 26
#define AVDB_SPLIT_OTHER 25
#define AVDB_SPLIT_NONE 0xFFu
#define AVDB_SPLIT_LINE_HOST 0x80000000u
#define AVDB_SPLIT_COUNT_LINES 0        /* 26 slots: the lines of stream c */
#define AVDB_SPLIT_COUNT_BYTES 26       /* 26 slots: the bytes of stream c */
#define AVDB_SPLIT_COUNT_COMMENTS 52
#define AVDB_SPLIT_COUNT_HOST_LINES 53
#define AVDB_SPLIT_COUNT_FIRST_OTHER 54
#define AVDB_SPLIT_N_COUNTS 55
int avdb_vcf_split_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes);
int avdb_vcf_split_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                        const avdb_chrom_map* chrom_map, uint8_t* code, uint64_t* line_start, uint32_t* out_len,
                        uint64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int avdb_vcf_split_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, const uint8_t* code,
                         const uint64_t* line_start, const uint32_t* out_len, uint8_t* out, size_t out_cap,
                         uint64_t* stream_off, uint64_t* dst_off, uint64_t* totals, void* workspace,
                         size_t workspace_bytes, void* stream);
int avdb_vcf_split_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                             const avdb_chrom_map* chrom_map, uint8_t* code, uint64_t* line_start, uint32_t* out_len,
                             uint64_t* counts);
int avdb_vcf_split_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                              const uint8_t* code, const uint64_t* line_start, const uint32_t* out_len, uint8_t* out,
                              size_t out_cap, uint64_t* stream_off, uint64_t* dst_off, uint64_t* totals);

/* ---- K9: genome-piece sharding of VCF text --------------------------------
 * The reference runs one process per chromosome file (Load/bin/load_vcf_file.py:
 * 307-313).  One file is split over the ranks of a node by a piece plan
 * (annotatedvdb_amd/shard.py: contigs cut at `cut` bp, pieces assigned to ranks):
 * piece_base[c] / piece_count[c] (host, one per contig) index piece_rank[]
 * (host, n_pieces <= 1024).  A K0 data line belongs to the rank owning the piece
 * that holds its POS (a POS past the contig end: its last piece); lines K0 could
 * not place (host-resolved CHROM/POS, empty or short lines) belong to rank 0;
 * comment lines to none.
 *   avdb_vcf_select_lines: sel_off[n_lines+1] = exclusive scan of this rank's
 *     bytes per line (line length + 1), total in sel_off[n_lines]; workspace of
 *     avdb_shard_workspace_size(n_lines) bytes.
 *   avdb_vcf_select_copy:  the rank's lines, each + '
', into out (sel_off[n_lines]
 *     bytes), in file order. */
int avdb_shard_workspace_size(size_t n_lines, size_t* bytes);
int avdb_vcf_select_lines(avdb_ctx* ctx, size_t n_lines, const avdb_vcf_line* lines,
                          const uint32_t* piece_base_host, const uint32_t* piece_count_host,
                          const uint8_t* piece_rank_host, uint32_t n_pieces, uint32_t cut, int rank,
                          void* workspace, size_t workspace_bytes, uint64_t* sel_off, void* stream);
int avdb_vcf_select_copy(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                         const avdb_vcf_line* lines, const uint64_t* sel_off, uint8_t* out, void* stream);

/* ---- node exchange over RCCL (SURVEY.md §8b avdb_hist_allgather, §8e) ------
 * The one collective of the path: every rank's L8 histogram (u32[n_bins], the
 * hist_l8 K1/K2 accumulate) and counters (u64[n_counters]) all-gathered in one
 * RCCL call (xGMI inside a node) and summed over the ranks on the device into
 * node_hist / node_counters.  The reference has no collective (one process per
 * chromosome file, Load/bin/load_vcf_file.py:307-313).  Rank 0 makes the id
 * with avdb_rccl_unique_id, hands its AVDB_RCCL_ID_BYTES bytes to the other
 * ranks out of band, and every rank calls avdb_rccl_comm_init with its rank.
 * RCCL is loaded at first use (dlopen); these calls return AVDB_ERCCL when it
 * is absent.  Workspace: avdb_hist_allgather_workspace_size, 8-byte aligned. */
#define AVDB_RCCL_ID_BYTES 128
int avdb_rccl_unique_id(void* id);
int avdb_rccl_comm_init(avdb_ctx* ctx, int world, int rank, const void* id, void** comm);
int avdb_rccl_comm_destroy(void* comm);
int avdb_hist_allgather_workspace_size(int world, size_t n_bins, size_t n_counters, size_t* bytes);
int avdb_hist_allgather(avdb_ctx* ctx, void* comm, const uint32_t* hist, size_t n_bins,
                        const uint64_t* counters, size_t n_counters, uint32_t* node_hist,
                        uint64_t* node_counters, void* workspace, size_t workspace_bytes, void* stream);

/* ---- K16: SnpEff LOF/NMD update rows (Load/bin/load_snpeff_lof.py) ---------
 * K16a, the table: `text` is a '\n'-separated slab of the VCF SnpEff wrote.  A line is read
 * as load_annotation reads it (:250-288): rstrip()ped; a '#' line is a comment; a line
 * without ';LOF=' and ';NMD=' anywhere in it is unannotated; of the others INFO is looked up
 * by key (the last item of a key wins), and a line with neither key counts no_values.  Every
 * other line is an entry: it yields one table row per ALT allele, the lookup id
 * chrom:pos:ref:alt (CHROM without `chr`, MT as M, POS without leading zeros) as the row's
 * key, and one JSON text, json.dumps({'LOF': [...], 'NMD': [...]}) of
 * parse_annotation_string's lists, shared by the line's rows.  An entry outside the device
 * subset is flagged AVDB_LOF_LINE_HOST: no rows, keys or JSON are counted
 * for it, the caller renders it, patches its alts / key_bytes / json_len and copies its
 * bytes into the spans the write pass leaves blank; AVDB_LOF_LINE_BAD marks the host lines
 * with fewer than eight fields.  A '\r' inside a stripped line is counted
 * (AVDB_LOF_COUNT_LONE_CR).
 *   1. avdb_lof_table_size: per entry (n_lines entries allocated, counts[ENTRIES] written)
 *      its line's offset, alts, key bytes, JSON length and flags; counts
 *      (AVDB_LOF_N_COUNTS x u64, set by the call).
 *   2. avdb_lof_table_write (n_entries as counted, n_rows = the sum of ent_alts, the same
 *      text): keys (key_cap bytes) with key_off[n_rows + 1], json (json_cap bytes), and per
 *      row the span of its line's JSON (row_json_off / row_json_len), its line's offset
 *      and flags (AVDB_LOF_ROW_FIRST on a line's first row, AVDB_LOF_LINE_HOST on a host
 *      line's rows, whose key_off all hold the line's first key's offset).  totals[0 .. 2]:
 *      the key bytes, JSON bytes and rows the entries add up to; totals[3]: 1 when any of
 *      them exceeds its capacity (nothing is written then; the _host form returns
 *      AVDB_ERANGE).  keys and json must be 8-byte aligned.
 * K16b, the update rows: `text` is a slab of an export
 * record_primary_key<TAB>metaseq_id<TAB>loss_of_function[<TAB>...] read by K13's conventions
 * (header line, fewer than two fields, contig mask, "\r\n", lone '\r').  A metaseq id
 * without exactly three ':' is a row flagged AVDB_LOFUPD_BAD (no output); the id's bytes are
 * probed in the table's key set: no hit counts NOT_ANNOTATED and is no row; a hit on row t
 * stores 1 to table->hit[t] and, unless the line's third field is present and neither empty
 * nor `\N` (counted SKIPPED, no row, without AVDB_LOFUPD_UPDATE_EXISTING), is the row
 * pk<TAB>chr<label of the metaseq id><TAB>json of t<LF>.
 * avdb_lof_table: the key set (avdb_keyset_build) is over the keys in REVERSE row order
 * (key i is row n_rows - 1 - i), so the last annotated record of an id answers.
 * Workspaces: avdb_lof_table_workspace_size / avdb_lof_update_workspace_size bytes, 256-byte
 * aligned; the device entries enqueue on `stream`, the _host forms run the same per-line code
 * on host arrays. */
#define AVDB_LOF_LINE_HOST 0x01u
#define AVDB_LOF_LINE_BAD 0x02u
#define AVDB_LOF_ROW_FIRST 0x04u
#define AVDB_LOF_COUNT_ROWS 0
#define AVDB_LOF_COUNT_LINES 1
#define AVDB_LOF_COUNT_COMMENT_LINES 2
#define AVDB_LOF_COUNT_UNANNOTATED_LINES 3
#define AVDB_LOF_COUNT_NO_VALUES 4
#define AVDB_LOF_COUNT_HOST_LINES 5
#define AVDB_LOF_COUNT_BAD 6
#define AVDB_LOF_COUNT_KEY_BYTES 7
#define AVDB_LOF_COUNT_JSON_BYTES 8
#define AVDB_LOF_COUNT_LONE_CR 9
#define AVDB_LOF_COUNT_ENTRIES 10
#define AVDB_LOF_N_COUNTS 11
#define AVDB_LOFUPD_BAD 0x02u
#define AVDB_LOFUPD_UPDATE_EXISTING 0x01u /* avdb_lof_update_size's flags */
#define AVDB_LOFUPD_COUNT_ROWS 0
#define AVDB_LOFUPD_COUNT_SKIPPED_LINES 1
#define AVDB_LOFUPD_COUNT_SKIPPED 2
#define AVDB_LOFUPD_COUNT_NOT_ANNOTATED 3
#define AVDB_LOFUPD_COUNT_BAD 4
#define AVDB_LOFUPD_COUNT_OUT_BYTES 5
#define AVDB_LOFUPD_COUNT_LONE_CR 6
#define AVDB_LOFUPD_N_COUNTS 7
typedef struct avdb_lof_table {
  uint32_t struct_size; /* sizeof(avdb_lof_table) */
  uint32_t reserved;
  uint64_t n_rows;
  const uint8_t* keys;     /* the rows' keys, in reverse row order */
  const uint64_t* key_off; /* n_rows + 1 */
  const void* keyset;      /* avdb_keyset_build over them */
  uint64_t keyset_bytes;
  const uint8_t* json;
  uint64_t json_bytes;
  const uint64_t* json_off; /* per row */
  const uint32_t* json_len;
  uint8_t* hit;             /* per row; NULL: not recorded */
} avdb_lof_table;
int avdb_lof_table_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes);
int avdb_lof_table_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, uint64_t* ent_start,
                        uint32_t* ent_alts, uint32_t* ent_key_bytes, uint32_t* ent_json_len, uint8_t* ent_flags,
                        uint64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int avdb_lof_table_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_entries,
                         size_t n_rows, const uint64_t* ent_start, const uint32_t* ent_alts,
                         const uint32_t* ent_key_bytes, const uint32_t* ent_json_len, const uint8_t* ent_flags,
                         uint8_t* keys, size_t key_cap, uint64_t* key_off, uint8_t* json, size_t json_cap,
                         uint64_t* row_json_off, uint32_t* row_json_len, uint64_t* row_line_start, uint8_t* row_flags,
                         uint64_t* totals, void* workspace, size_t workspace_bytes, void* stream);
int avdb_lof_table_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                             uint64_t* ent_start, uint32_t* ent_alts, uint32_t* ent_key_bytes, uint32_t* ent_json_len,
                             uint8_t* ent_flags, uint64_t* counts);
int avdb_lof_table_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                              size_t n_entries, size_t n_rows, const uint64_t* ent_start, const uint32_t* ent_alts,
                              const uint32_t* ent_key_bytes, const uint32_t* ent_json_len, const uint8_t* ent_flags,
                              uint8_t* keys, size_t key_cap, uint64_t* key_off, uint8_t* json, size_t json_cap,
                              uint64_t* row_json_off, uint32_t* row_json_len, uint64_t* row_line_start,
                              uint8_t* row_flags, uint64_t* totals);
int avdb_lof_update_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes);
int avdb_lof_update_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                         const avdb_lof_table* table, uint32_t contig_mask, uint32_t flags, uint64_t* row_start,
                         uint32_t* pk_len, int32_t* match, uint32_t* out_len, uint8_t* row_flags, uint64_t* counts,
                         void* workspace, size_t workspace_bytes, void* stream);
int avdb_lof_update_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_rows,
                          const avdb_lof_table* table, const uint64_t* row_start, const uint32_t* pk_len,
                          const int32_t* match, const uint32_t* out_len, const uint8_t* row_flags, uint8_t* out,
                          size_t out_cap, uint64_t* row_off, uint64_t* totals, void* workspace, size_t workspace_bytes,
                          void* stream);
int avdb_lof_update_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                              const avdb_lof_table* table, uint32_t contig_mask, uint32_t flags, uint64_t* row_start,
                              uint32_t* pk_len, int32_t* match, uint32_t* out_len, uint8_t* row_flags,
                              uint64_t* counts);
int avdb_lof_update_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                               size_t n_rows, const avdb_lof_table* table, const uint64_t* row_start,
                               const uint32_t* pk_len, const int32_t* match, const uint32_t* out_len,
                               const uint8_t* row_flags, uint8_t* out, size_t out_cap, uint64_t* row_off,
                               uint64_t* totals);

/* ---- K17: ADSP QC pVCF update rows (Load/bin/update_from_qc_pvcf_file.py) ----
 * K17a, the table: `text` is a '\n'-separated slab of an ADSP QC pVCF.  A line is read as
 * load_annotation reads it (:226-258): rstrip()ped; a '#' line is a comment; every other line
 * is an entry, read by the header #CHROM .. FORMAT (nine fields; columns beyond the ninth are
 * ignored).  An entry yields one table row per ALT allele, the lookup id chrom:pos:ref:alt as
 * the row's key (as K16a), and one JSON text shared by the line's rows,
 *   json.dumps({release: {"info": {...}, "filter": v, "qual": v, "format": v}})
 * with INFO as parse_entry splits it (a bare flag is true, '#' reads ':') and every value as
 * to_numeric leaves it.  `release` (1 .. AVDB_QC_RELEASE_MAX bytes, none of them '"', '\',
 * a control byte or above 0x7F) is written as it is.  AVDB_QC_PASS marks an entry whose FILTER
 * is exactly PASS.  An entry outside the device subset is flagged
 * AVDB_QC_LINE_HOST and treated as K16a treats its host lines; AVDB_QC_LINE_BAD marks the host
 * lines with fewer than nine fields.
 *   1. avdb_qc_table_size, 2. avdb_qc_table_write: the arrays, totals and alignment of
 *      avdb_lof_table_size / avdb_lof_table_write; row_flags hold AVDB_QC_ROW_FIRST,
 *      AVDB_QC_LINE_HOST and AVDB_QC_PASS.
 * K17b, the update rows: `text` is a slab of an export
 * record_primary_key<TAB>metaseq_id<TAB>adsp_qc[<TAB>...] read by K13's conventions.  The id
 * is probed as in K16b: no hit counts NOT_IN_VCF; a hit on row t stores 1 to table->hit[t] and
 * is the row pk<TAB>chr<label><TAB>true|\N<TAB>json of t<LF> (true: row t has AVDB_QC_PASS),
 * unless, without AVDB_QCUPD_UPDATE_EXISTING, the third field is not NULL (absent, empty, \N)
 * and a key at depth 1 of its JSON object equals the release (counted SKIPPED, no row).  A third
 * field that holds a '\' or does not begin with '{' makes the row AVDB_QCUPD_ROW_HOST: it is
 * sized and written as an update row and the caller settles whether it is one.
 * avdb_qc_table: avdb_lof_table's members, the rows' flags and the release. */
#define AVDB_QC_LINE_HOST 0x01u
#define AVDB_QC_LINE_BAD 0x02u
#define AVDB_QC_ROW_FIRST 0x04u
#define AVDB_QC_PASS 0x08u
#define AVDB_QC_RELEASE_MAX 64
#define AVDB_QC_COUNT_ROWS 0
#define AVDB_QC_COUNT_LINES 1
#define AVDB_QC_COUNT_COMMENT_LINES 2
#define AVDB_QC_COUNT_HOST_LINES 3
#define AVDB_QC_COUNT_BAD 4
#define AVDB_QC_COUNT_KEY_BYTES 5
#define AVDB_QC_COUNT_JSON_BYTES 6
#define AVDB_QC_COUNT_LONE_CR 7
#define AVDB_QC_COUNT_ENTRIES 8
#define AVDB_QC_COUNT_PASS 9
#define AVDB_QC_N_COUNTS 10
#define AVDB_QCUPD_ROW_HOST 0x01u
#define AVDB_QCUPD_BAD 0x02u
#define AVDB_QCUPD_UPDATE_EXISTING 0x01u /* avdb_qc_update_size's flags */
#define AVDB_QCUPD_COUNT_ROWS 0
#define AVDB_QCUPD_COUNT_SKIPPED_LINES 1
#define AVDB_QCUPD_COUNT_SKIPPED 2
#define AVDB_QCUPD_COUNT_NOT_IN_VCF 3
#define AVDB_QCUPD_COUNT_BAD 4
#define AVDB_QCUPD_COUNT_OUT_BYTES 5
#define AVDB_QCUPD_COUNT_LONE_CR 6
#define AVDB_QCUPD_COUNT_HOST_ROWS 7
#define AVDB_QCUPD_N_COUNTS 8
typedef struct avdb_qc_table {
  uint32_t struct_size; /* sizeof(avdb_qc_table) */
  uint32_t release_len;
  uint64_t n_rows;
  const uint8_t* keys;     /* the rows' keys, in reverse row order */
  const uint64_t* key_off; /* n_rows + 1 */
  const void* keyset;      /* avdb_keyset_build over them */
  uint64_t keyset_bytes;
  const uint8_t* json;
  uint64_t json_bytes;
  const uint64_t* json_off; /* per row */
  const uint32_t* json_len;
  const uint8_t* flags;     /* per row: AVDB_QC_PASS */
  uint8_t* hit;             /* per row; NULL: not recorded */
  const uint8_t* release;   /* host memory, release_len bytes */
} avdb_qc_table;
int avdb_qc_table_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes);
int avdb_qc_table_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, const uint8_t* release,
                       size_t release_len, uint64_t* ent_start, uint32_t* ent_alts, uint32_t* ent_key_bytes,
                       uint32_t* ent_json_len, uint8_t* ent_flags, uint64_t* counts, void* workspace,
                       size_t workspace_bytes, void* stream);
int avdb_qc_table_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_entries,
                        size_t n_rows, const uint8_t* release, size_t release_len, const uint64_t* ent_start,
                        const uint32_t* ent_alts, const uint32_t* ent_key_bytes, const uint32_t* ent_json_len,
                        const uint8_t* ent_flags, uint8_t* keys, size_t key_cap, uint64_t* key_off, uint8_t* json,
                        size_t json_cap, uint64_t* row_json_off, uint32_t* row_json_len, uint64_t* row_line_start,
                        uint8_t* row_flags, uint64_t* totals, void* workspace, size_t workspace_bytes, void* stream);
int avdb_qc_table_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                            const uint8_t* release, size_t release_len, uint64_t* ent_start, uint32_t* ent_alts,
                            uint32_t* ent_key_bytes, uint32_t* ent_json_len, uint8_t* ent_flags, uint64_t* counts);
int avdb_qc_table_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                             size_t n_entries, size_t n_rows, const uint8_t* release, size_t release_len,
                             const uint64_t* ent_start, const uint32_t* ent_alts, const uint32_t* ent_key_bytes,
                             const uint32_t* ent_json_len, const uint8_t* ent_flags, uint8_t* keys, size_t key_cap,
                             uint64_t* key_off, uint8_t* json, size_t json_cap, uint64_t* row_json_off,
                             uint32_t* row_json_len, uint64_t* row_line_start, uint8_t* row_flags, uint64_t* totals);
int avdb_qc_update_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes);
int avdb_qc_update_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                        const avdb_qc_table* table, uint32_t contig_mask, uint32_t flags, uint64_t* row_start,
                        uint32_t* pk_len, int32_t* match, uint32_t* out_len, uint8_t* row_flags, uint64_t* counts,
                        void* workspace, size_t workspace_bytes, void* stream);
int avdb_qc_update_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_rows,
                         const avdb_qc_table* table, const uint64_t* row_start, const uint32_t* pk_len,
                         const int32_t* match, const uint32_t* out_len, const uint8_t* row_flags, uint8_t* out,
                         size_t out_cap, uint64_t* row_off, uint64_t* totals, void* workspace, size_t workspace_bytes,
                         void* stream);
int avdb_qc_update_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                             const avdb_qc_table* table, uint32_t contig_mask, uint32_t flags, uint64_t* row_start,
                             uint32_t* pk_len, int32_t* match, uint32_t* out_len, uint8_t* row_flags,
                             uint64_t* counts);
int avdb_qc_update_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                              size_t n_rows, const avdb_qc_table* table, const uint64_t* row_start,
                              const uint32_t* pk_len, const int32_t* match, const uint32_t* out_len,
                              const uint8_t* row_flags, uint8_t* out, size_t out_cap, uint64_t* row_off,
                              uint64_t* totals);

/* ---- K19: annotation update rows from a tab-delimited file (Load/bin/update_variant_annotation.py) ----
 * `text` is a '\n'-separated slab of a tab-delimited file with a header.  The header is the
 * caller's (csv's own parse): skip_lines is the number of the slab's lines up to and including
 * it, n_fields (2 .. AVDB_TXT_MAX_FIELDS) its field count, id_col the field named `variant`,
 * key_col the field that is looked up (id_col, or the `ref_snp_id` column for refSNP ids).  A
 * line behind the header is a data line unless it is empty ("\r\n" ends a line too; a '\r'
 * elsewhere is counted LONE_CR).  Its update values ("tail") are its first n_fields fields
 * without field id_col, joined by tabs: a field that is exactly NULL, and a field a short line
 * lacks, reads \N; fields beyond n_fields are dropped.  Its chromosome is chr<label>, the label
 * being the id up to its first ':', or, for an id without one, the primary key up to its first
 * ':'.  A data line outside the device subset is flagged AVDB_TXT_LINE_HOST and left to the
 * caller: a field that starts with '"', a byte above 0x7F, a field that is exactly \N;
 * AVDB_TXT_LINE_BAD as well for a line that lacks field id_col or key_col or whose looked-up
 * field is empty.
 * K19a, the table (one row per data line, the arrays, totals and alignment of
 * avdb_lof_table_size / avdb_lof_table_write; ent_alts is 1, or 0 for a host line until the
 * caller patches it): the row's key is its looked-up field, its body <label><TAB><tail>, the
 * label left out and AVDB_TXT_ROW_PK_CHROM set when the id has no ':'.
 * K19b, the update rows: `text` is a slab of an export
 * record_primary_key<TAB>metaseq_id<TAB>ref_snp_id[<TAB>...] read by K13's conventions (header
 * line, fewer than two fields, contig mask by the metaseq id, a metaseq id without exactly three
 * ':' is a row flagged AVDB_TXTUPD_BAD).  Field key_col (1: metaseq_id; 2: ref_snp_id, none
 * when absent, empty or \N) is probed in the table's key set: no hit counts NOT_IN_FILE; a hit
 * on row t stores 1 to table->hit[t] and is the row pk<TAB>chr<label><TAB><tail>[<TAB>true]<LF>
 * (`true` with AVDB_TXT_ADSP in flags).  AVDB_TXTUPD_TABLE_HOST marks a row of a host-rendered
 * table row.  avdb_txt_table: as avdb_lof_table, the keys in REVERSE row order, so the last line
 * of a repeated id answers.
 * K19c, a file whose `variant` column holds primary keys: every data line is the row
 * pk<TAB>chr<label><TAB><tail>[<TAB>true]<LF>, in file order; a host line is a row of no bytes
 * whose out_len the caller patches and whose span it fills.
 * Workspaces: avdb_txt_*_workspace_size bytes, 256-byte aligned; outputs 8-byte aligned; the
 * device entries enqueue on `stream`, the _host forms run the same per-line code on host arrays. */
#define AVDB_TXT_MAX_FIELDS 32
#define AVDB_TXT_LINE_HOST 0x01u
#define AVDB_TXT_LINE_BAD 0x02u
#define AVDB_TXT_ROW_PK_CHROM 0x04u
#define AVDB_TXT_ADSP 0x01u /* the update and direct entries' flags */
#define AVDB_TXT_COUNT_ROWS 0
#define AVDB_TXT_COUNT_LINES 1
#define AVDB_TXT_COUNT_SKIPPED_LINES 2
#define AVDB_TXT_COUNT_HOST_LINES 3
#define AVDB_TXT_COUNT_BAD 4
#define AVDB_TXT_COUNT_KEY_BYTES 5
#define AVDB_TXT_COUNT_JSON_BYTES 6 /* the bodies' bytes (the slot K16a and K17a name so) */
#define AVDB_TXT_COUNT_LONE_CR 7
#define AVDB_TXT_COUNT_ENTRIES 8
#define AVDB_TXT_N_COUNTS 9
#define AVDB_TXTUPD_TABLE_HOST 0x01u
#define AVDB_TXTUPD_BAD 0x02u
#define AVDB_TXTUPD_COUNT_ROWS 0
#define AVDB_TXTUPD_COUNT_SKIPPED_LINES 1
#define AVDB_TXTUPD_COUNT_NOT_IN_FILE 2
#define AVDB_TXTUPD_COUNT_BAD 3
#define AVDB_TXTUPD_COUNT_OUT_BYTES 4
#define AVDB_TXTUPD_COUNT_LONE_CR 5
#define AVDB_TXTUPD_COUNT_HOST_ROWS 6
#define AVDB_TXTUPD_N_COUNTS 7
#define AVDB_TXTDIR_COUNT_ROWS 0
#define AVDB_TXTDIR_COUNT_LINES 1
#define AVDB_TXTDIR_COUNT_SKIPPED_LINES 2
#define AVDB_TXTDIR_COUNT_HOST_ROWS 3
#define AVDB_TXTDIR_COUNT_BAD 4
#define AVDB_TXTDIR_COUNT_OUT_BYTES 5
#define AVDB_TXTDIR_COUNT_LONE_CR 6
#define AVDB_TXTDIR_N_COUNTS 7
typedef struct avdb_txt_table {
  uint32_t struct_size; /* sizeof(avdb_txt_table) */
  uint32_t reserved;
  uint64_t n_rows;
  const uint8_t* keys;     /* the rows' keys, in reverse row order */
  const uint64_t* key_off; /* n_rows + 1 */
  const void* keyset;      /* avdb_keyset_build over them */
  uint64_t keyset_bytes;
  const uint8_t* body;
  uint64_t body_bytes;
  const uint64_t* body_off; /* per row */
  const uint32_t* body_len;
  const uint8_t* flags;     /* per row: AVDB_TXT_ROW_PK_CHROM, AVDB_TXT_LINE_HOST */
  uint8_t* hit;             /* per row; NULL: not recorded */
} avdb_txt_table;
int avdb_txt_table_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes);
int avdb_txt_table_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, uint32_t skip_lines,
                        uint32_t n_fields, uint32_t id_col, uint32_t key_col, uint64_t* ent_start, uint32_t* ent_alts,
                        uint32_t* ent_key_bytes, uint32_t* ent_body_len, uint8_t* ent_flags, uint64_t* counts,
                        void* workspace, size_t workspace_bytes, void* stream);
int avdb_txt_table_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_entries,
                         size_t n_rows, uint32_t skip_lines, uint32_t n_fields, uint32_t id_col, uint32_t key_col,
                         const uint64_t* ent_start, const uint32_t* ent_alts, const uint32_t* ent_key_bytes,
                         const uint32_t* ent_body_len, const uint8_t* ent_flags, uint8_t* keys, size_t key_cap,
                         uint64_t* key_off, uint8_t* body, size_t body_cap, uint64_t* row_body_off,
                         uint32_t* row_body_len, uint64_t* row_line_start, uint8_t* row_flags, uint64_t* totals,
                         void* workspace, size_t workspace_bytes, void* stream);
int avdb_txt_table_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                             uint32_t skip_lines, uint32_t n_fields, uint32_t id_col, uint32_t key_col,
                             uint64_t* ent_start, uint32_t* ent_alts, uint32_t* ent_key_bytes, uint32_t* ent_body_len,
                             uint8_t* ent_flags, uint64_t* counts);
int avdb_txt_table_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                              size_t n_entries, size_t n_rows, uint32_t skip_lines, uint32_t n_fields, uint32_t id_col,
                              uint32_t key_col, const uint64_t* ent_start, const uint32_t* ent_alts,
                              const uint32_t* ent_key_bytes, const uint32_t* ent_body_len, const uint8_t* ent_flags,
                              uint8_t* keys, size_t key_cap, uint64_t* key_off, uint8_t* body, size_t body_cap,
                              uint64_t* row_body_off, uint32_t* row_body_len, uint64_t* row_line_start,
                              uint8_t* row_flags, uint64_t* totals);
int avdb_txt_update_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes);
int avdb_txt_update_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                         const avdb_txt_table* table, uint32_t contig_mask, uint32_t key_col, uint32_t flags,
                         uint64_t* row_start, uint32_t* pk_len, int32_t* match, uint32_t* out_len, uint8_t* row_flags,
                         uint64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int avdb_txt_update_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_rows,
                          const avdb_txt_table* table, uint32_t flags, const uint64_t* row_start,
                          const uint32_t* pk_len, const int32_t* match, const uint32_t* out_len,
                          const uint8_t* row_flags, uint8_t* out, size_t out_cap, uint64_t* row_off, uint64_t* totals,
                          void* workspace, size_t workspace_bytes, void* stream);
int avdb_txt_update_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                              const avdb_txt_table* table, uint32_t contig_mask, uint32_t key_col, uint32_t flags,
                              uint64_t* row_start, uint32_t* pk_len, int32_t* match, uint32_t* out_len,
                              uint8_t* row_flags, uint64_t* counts);
int avdb_txt_update_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                               size_t n_rows, const avdb_txt_table* table, uint32_t flags, const uint64_t* row_start,
                               const uint32_t* pk_len, const int32_t* match, const uint32_t* out_len,
                               const uint8_t* row_flags, uint8_t* out, size_t out_cap, uint64_t* row_off,
                               uint64_t* totals);
int avdb_txt_direct_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes);
int avdb_txt_direct_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, uint32_t skip_lines,
                         uint32_t n_fields, uint32_t id_col, uint32_t flags, uint64_t* row_start, uint32_t* out_len,
                         uint8_t* row_flags, uint64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int avdb_txt_direct_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_rows,
                          uint32_t skip_lines, uint32_t n_fields, uint32_t id_col, uint32_t flags,
                          const uint64_t* row_start, const uint32_t* out_len, const uint8_t* row_flags, uint8_t* out,
                          size_t out_cap, uint64_t* row_off, uint64_t* totals, void* workspace, size_t workspace_bytes,
                          void* stream);
int avdb_txt_direct_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                              uint32_t skip_lines, uint32_t n_fields, uint32_t id_col, uint32_t flags,
                              uint64_t* row_start, uint32_t* out_len, uint8_t* row_flags, uint64_t* counts);
int avdb_txt_direct_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                               size_t n_rows, uint32_t skip_lines, uint32_t n_fields, uint32_t id_col, uint32_t flags,
                               const uint64_t* row_start, const uint32_t* out_len, const uint8_t* row_flags,
                               uint8_t* out, size_t out_cap, uint64_t* row_off, uint64_t* totals);

/* ---- K18a: the consequences of VEP's JSON lines, ranked and sorted ---------------------------
 * `text` is a '\n'-separated slab of VEP --json output: one compact JSON object a line ("\r\n"
 * ends a line too).  For every element of the line's four <type>_consequences arrays (transcript,
 * regulatory_feature, motif_feature, intergenic: types 0..3) the pass gives what
 * VepJsonParser.adsp_rank_and_sort_consequences adds (vep_parser.py:145-175): its index in its
 * array (vep_consequence_order_num), the ranking entry of its consequence_terms (rank) and whether
 * one of them is a coding term (consequence_is_coding); and the order the elements end up in: type,
 * then the variant_allele's first appearance in the array, then (rank, index).  One wave reads a
 * line, 64 bytes a step.
 * avdb_vep_table: the ranking.  Term i is term_len[i] bytes, zero-padded to whole words at
 * term_words[term_off[i]]; at most 64 terms.  A combination is the mask of its terms' numbers; the
 * open-addressed slots (n_slots a power of two, slot_entry -1 for none, avdb_vep_table_build fills
 * them on the host) map a mask to its ranking entry, rank_order[entry] is the entry's place among
 * the distinct ranks, coding_mask the coding terms.  The arrays live where the entry runs.
 *   1. avdb_vep_index_size: per line its consequences n_csq, a flags byte, `types` (bit t: the line
 *      has the <type>_consequences key of type t, were its array empty), and the spans of the
 *      top-level strings `input` and `id` (the bytes between the quotes; length -1: none); counts
 *      (AVDB_VEP_N_COUNTS x u64, set by the call).  flags 0: the device answers the line; else 1 +
 *      the first of the reasons it is left to the caller, counted under AVDB_VEP_COUNT_REASON0 +
 *      reason: 0 whitespace outside a string, 1 no '{' first or brackets or a string left open, 2
 *      depth beyond AVDB_VEP_MAX_DEPTH, 3 a key of interest twice at the top level, 4 an element
 *      that is no object with one variant_allele string and one consequence_terms array of strings
 *      (or a <type>_consequences value that is no array of objects), 5 a backslash or a byte >=
 *      0x80 in a key, an allele or a term, 6 a term twice in one element, 7 no terms, 8 a term the
 *      table lacks, 9 a combination it lacks, 10 more than AVDB_VEP_MAX_CSQ consequences.  JSON
 *      grammar is not checked beyond this.
 *   2. avdb_vep_index_write (csq_off: the exclusive sums of n_csq, n_csq_total their sum): row
 *      csq_off[line] + k is the line's k-th consequence in text order: type, order number, the
 *      element's span, the allele's span, term mask, ranking entry, coding flag.  sorted[csq_off
 *      [line] + p] is the k of the consequence at place p of the order above, head[...+ p] 1 when
 *      it is the first of its (type, allele) group.  A line with flags != 0 gets blank rows (entry
 *      -1, sorted the identity).  totals[0]: rows written, totals[1]: lines whose count differs
 *      from n_csq or whose rows do not fit (nothing is written for them).
 * Workspace: avdb_vep_index_workspace_size bytes, 256-byte aligned; the device entries enqueue on
 * `stream`, the _host forms run the same per-block code on host arrays. */
#define AVDB_VEP_MAX_CSQ 512   /* consequences of a line the device sorts (quadratic per line, 20 KiB of LDS per wave) */
#define AVDB_VEP_MAX_DEPTH 64
#define AVDB_VEP_GRID_WAVES 2048 /* at most this many waves (one a workgroup) read a slab: wave w the lines w, w + waves, ... */
#define AVDB_VEP_N_REASONS 11
#define AVDB_VEP_COUNT_LINES 0
#define AVDB_VEP_COUNT_HOST_LINES 1
#define AVDB_VEP_COUNT_CSQ 2
#define AVDB_VEP_COUNT_REASON0 3
#define AVDB_VEP_N_COUNTS 14
typedef struct avdb_vep_table {
  uint32_t struct_size; /* sizeof(avdb_vep_table) */
  uint32_t n_terms;
  const uint64_t* term_words;
  const uint32_t* term_off; /* per term, in words */
  const uint32_t* term_len; /* per term, in bytes */
  const uint64_t* slot_mask;
  const int32_t* slot_entry;
  uint32_t n_slots;
  uint32_t n_entries;
  const uint32_t* rank_order; /* per entry */
  uint64_t coding_mask;
} avdb_vep_table;
/* host arrays: the slots of n_entries masks (the first entry of a mask stays); AVDB_EINVAL for more
 * than 64 terms, a mask with a term beyond n_terms, or fewer than 2 * n_entries slots */
int avdb_vep_table_build(const avdb_ctx* ctx, uint32_t n_terms, const uint64_t* entry_mask, size_t n_entries,
                         uint64_t* slot_mask, int32_t* slot_entry, size_t n_slots);
int avdb_vep_index_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes);
int avdb_vep_index_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                        const avdb_vep_table* table, uint32_t* n_csq, uint8_t* flags, uint8_t* types, uint64_t* input_start,
                        int32_t* input_len, uint64_t* id_start, int32_t* id_len, uint64_t* counts, void* workspace,
                        size_t workspace_bytes, void* stream);
int avdb_vep_index_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                         const avdb_vep_table* table, const uint32_t* n_csq, const uint8_t* flags,
                         const uint64_t* csq_off, size_t n_csq_total, uint8_t* type, int32_t* order,
                         uint64_t* el_start, uint32_t* el_len, uint64_t* al_start, uint32_t* al_len, uint64_t* mask,
                         int32_t* entry, uint8_t* coding, int32_t* sorted, uint8_t* head, uint64_t* totals,
                         void* workspace, size_t workspace_bytes, void* stream);
int avdb_vep_index_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                             const avdb_vep_table* table, uint32_t* n_csq, uint8_t* flags, uint8_t* types, uint64_t* input_start,
                             int32_t* input_len, uint64_t* id_start, int32_t* id_len, uint64_t* counts);
int avdb_vep_index_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                              const avdb_vep_table* table, const uint32_t* n_csq, const uint8_t* flags,
                              const uint64_t* csq_off, size_t n_csq_total, uint8_t* type, int32_t* order,
                              uint64_t* el_start, uint32_t* el_len, uint64_t* al_start, uint32_t* al_len,
                              uint64_t* mask, int32_t* entry, uint8_t* coding, int32_t* sorted, uint8_t* head,
                              uint64_t* totals);

/* ---- K18b: VEP consequence update rows (Load/bin/load_vep_result.py, two of its four columns) ----
 * The update rows for adsp_most_severe_consequence and adsp_ranked_consequences of VEPVariantLoader
 * (vep_variant_loader.py:153-213), on K18a's arrays of the same slab and K16's two-half shape.
 * Table build: every line is an entry.  A line the device answers gives one row per ALT allele of
 * the VCF line in its top-level `input` string (its first five fields, separated by the two bytes
 * \t): the row's key is the metaseq id chrom:pos:ref:alt (CHROM without 'chr', MT as M, POS without
 * leading zeros), its body <most severe><TAB><ranked>: json.dumps of get_most_severe_consequence
 * (normAlt) and of get_allele_consequences(normAlt), '{}' for None, normAlt the ALT without the
 * prefix it shares with REF ('-' when nothing is left; an SNV as it is).  An element is rendered
 * from its own bytes: a space behind every ',' and ':' outside strings, and
 * `, "vep_consequence_order_num": k, "rank": r, "consequence_is_coding": true|false` before its
 * closing brace; r is entry e's text rank_text[rank_off[e] .. rank_off[e + 1]).  A line outside the
 * device subset is flagged AVDB_VEPROWS_LINE_HOST (no rows, keys or body counted; the caller
 * patches ent_alts, ent_key_bytes and ent_json_len and copies its bytes in after the write pass):
 * K18a's reasons 0 .. 10, then 11 no `input` string, 12 `input` with fewer than five fields, a
 * backslash other than the separators' or a field outside K16's first-five-field subset, 13 a
 * backslash escape other than \" \\ \b \f \n \r \t in an element, 14 a byte >= 0x80 or < 0x20 in
 * an element, 15 a token outside strings that is not true, false, null, an integer without a
 * leading zero (not -0), or -?int.frac of at most 15 significant digits without a trailing zero
 * (a fraction of exactly 0 excepted) and of magnitude in [1e-4, 1e16), of at most 32 bytes.  The
 * first reason r is counted under AVDB_VEPROWS_COUNT_REASON0 + r and kept in the entry's flags as
 * (r + 1) << 2.
 *   1. avdb_vep_rows_table_size: el_rlen[c] for every consequence of a line K18a answered (its
 *      rendered length, or 0x80000000 | reason), then per entry its columns as avdb_lof_table_size.
 *   2. avdb_vep_rows_table_write: as avdb_lof_table_write; a row's json_off / json_len is its own
 *      body, an entry's ent_json_len their sum.
 * Export join (avdb_vep_rows_update_size / _write): avdb_lof_update_size's export, table view,
 * counts (AVDB_LOFUPD_COUNT_*), row flags and conventions, the third column being vep_output; a
 * row is pk<TAB>chr<label><TAB>body<TAB>alg_id[<TAB>true]<LF>, `true` with AVDB_VEPUPD_ADSP. */
#define AVDB_VEPROWS_LINE_HOST 0x01u
#define AVDB_VEPROWS_LINE_BAD 0x02u /* (no line is) */
#define AVDB_VEPROWS_ROW_FIRST 0x04u
#define AVDB_VEPROWS_N_REASONS 16
#define AVDB_VEPROWS_MAX_TOKEN 32
#define AVDB_VEPROWS_COUNT_ROWS 0
#define AVDB_VEPROWS_COUNT_LINES 1
#define AVDB_VEPROWS_COUNT_HOST_LINES 2
#define AVDB_VEPROWS_COUNT_BAD 3
#define AVDB_VEPROWS_COUNT_KEY_BYTES 4
#define AVDB_VEPROWS_COUNT_JSON_BYTES 5
#define AVDB_VEPROWS_COUNT_LONE_CR 6 /* always 0: K18a drops a line's last '\r', any other sends the line to the host */
#define AVDB_VEPROWS_COUNT_ENTRIES 7
#define AVDB_VEPROWS_COUNT_REASON0 8
#define AVDB_VEPROWS_N_COUNTS 24
#define AVDB_VEPUPD_UPDATE_EXISTING 0x01u /* avdb_vep_rows_update_size's flags */
#define AVDB_VEPUPD_ADSP 0x02u            /* ... and avdb_vep_rows_update_write's */
typedef struct avdb_vep_rows_in {
  uint32_t struct_size; /* sizeof(avdb_vep_rows_in) */
  uint32_t n_ranks;     /* the ranking's entries */
  uint64_t n_csq_total;
  const uint8_t* rank_text;
  uint64_t rank_text_bytes;
  const uint32_t* rank_off; /* n_ranks + 1 */
  /* per line, as avdb_vep_index_size left them (csq_off: the caller's sums) */
  const uint8_t* line_flags;
  const uint32_t* n_csq;
  const uint64_t* csq_off;
  const uint64_t* input_start;
  const int32_t* input_len;
  /* per consequence, as avdb_vep_index_write left them */
  const uint8_t* type;
  const int32_t* order;
  const uint64_t* el_start;
  const uint32_t* el_len;
  const uint64_t* al_start;
  const uint32_t* al_len;
  const int32_t* entry;
  const uint8_t* coding;
  const int32_t* sorted;
  uint32_t* el_rlen; /* per consequence: written by the size entry, read by the write entry */
} avdb_vep_rows_in;
typedef avdb_lof_table avdb_vep_rows_table;
int avdb_vep_rows_table_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes);
int avdb_vep_rows_table_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                             const avdb_vep_rows_in* in, uint64_t* ent_start, uint32_t* ent_alts,
                             uint32_t* ent_key_bytes, uint32_t* ent_json_len, uint8_t* ent_flags, uint64_t* counts,
                             void* workspace, size_t workspace_bytes, void* stream);
int avdb_vep_rows_table_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_entries,
                              size_t n_rows, const avdb_vep_rows_in* in, const uint64_t* ent_start,
                              const uint32_t* ent_alts, const uint32_t* ent_key_bytes, const uint32_t* ent_json_len,
                              const uint8_t* ent_flags, uint8_t* keys, size_t key_cap, uint64_t* key_off, uint8_t* json,
                              size_t json_cap, uint64_t* row_json_off, uint32_t* row_json_len, uint64_t* row_line_start,
                              uint8_t* row_flags, uint64_t* totals, void* workspace, size_t workspace_bytes,
                              void* stream);
int avdb_vep_rows_table_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                  const avdb_vep_rows_in* in, uint64_t* ent_start, uint32_t* ent_alts,
                                  uint32_t* ent_key_bytes, uint32_t* ent_json_len, uint8_t* ent_flags,
                                  uint64_t* counts);
int avdb_vep_rows_table_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                   size_t n_entries, size_t n_rows, const avdb_vep_rows_in* in,
                                   const uint64_t* ent_start, const uint32_t* ent_alts, const uint32_t* ent_key_bytes,
                                   const uint32_t* ent_json_len, const uint8_t* ent_flags, uint8_t* keys,
                                   size_t key_cap, uint64_t* key_off, uint8_t* json, size_t json_cap,
                                   uint64_t* row_json_off, uint32_t* row_json_len, uint64_t* row_line_start,
                                   uint8_t* row_flags, uint64_t* totals);
/* 1 when the n bytes are a token the device copies (reason 15's rule), else 0 */
int avdb_vep_rows_token_ok_host(const uint8_t* token, size_t n);
int avdb_vep_rows_update_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes);
int avdb_vep_rows_update_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                              const avdb_vep_rows_table* table, uint32_t contig_mask, uint32_t flags, uint64_t alg_id,
                              uint64_t* row_start, uint32_t* pk_len, int32_t* match, uint32_t* out_len,
                              uint8_t* row_flags, uint64_t* counts, void* workspace, size_t workspace_bytes,
                              void* stream);
int avdb_vep_rows_update_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_rows,
                               const avdb_vep_rows_table* table, uint32_t flags, uint64_t alg_id,
                               const uint64_t* row_start, const uint32_t* pk_len, const int32_t* match,
                               const uint32_t* out_len, const uint8_t* row_flags, uint8_t* out, size_t out_cap,
                               uint64_t* row_off, uint64_t* totals, void* workspace, size_t workspace_bytes,
                               void* stream);
int avdb_vep_rows_update_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                   const avdb_vep_rows_table* table, uint32_t contig_mask, uint32_t flags,
                                   uint64_t alg_id, uint64_t* row_start, uint32_t* pk_len, int32_t* match,
                                   uint32_t* out_len, uint8_t* row_flags, uint64_t* counts);
int avdb_vep_rows_update_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                    size_t n_rows, const avdb_vep_rows_table* table, uint32_t flags, uint64_t alg_id,
                                    const uint64_t* row_start, const uint32_t* pk_len, const int32_t* match,
                                    const uint32_t* out_len, const uint8_t* row_flags, uint8_t* out, size_t out_cap,
                                    uint64_t* row_off, uint64_t* totals);

/* ---- K18c: the vep_output column of the VEP update rows ---------------------------------------
 * xstr(cleanResult) of VEPVariantLoader.__parse_alt_alleles (vep_variant_loader.py:112-123, 202),
 * the same text for every ALT of a line: the line's top-level object with the members
 * colocated_variants and the four <type>_consequences removed, the value of `input` replaced by
 * VcfEntryParser's entry dict (vcf_parser.py:76-114: chrom pos id ref alt, and qual filter info
 * unless AVDB_VEPOUT_IDENTITY_ONLY), printed as json.dumps prints it.  On K18a's arrays of the same
 * slab (avdb_vep_rows_in; el_rlen is not read) and K18b's entry flags (entry e is line e).
 *   1. avdb_vep_output_size: per line its start, the length of its cleaned text, where the entry
 *      dict begins in it and the dict's length, and a flags byte: 0, or 1 + the reason the line is
 *      left to the caller (lengths 0): a reason of K18a or K18b (0 .. 15, as the entry's flags keep
 *      it), 16 a kept member with a backslash escape, a byte or a token outside K18b's element
 *      subset (reasons 13 .. 15, over the whole kept text; a byte < 0x20 anywhere in the line), 17
 *      fewer than eight fields in `input` without AVDB_VEPOUT_IDENTITY_ONLY, 18 a field or an INFO
 *      value outside K17's device forms (avdb_qc_table_size), a backslash other than the
 *      separators', a byte json.dumps escapes, an INFO that to_numeric turns into a number or
 *      that repeats a key.  counts: AVDB_VEPOUT_N_COUNTS x u64, set by the call.
 *   2. avdb_vep_output_write (out_off: the caller's offsets; a line with flags != 0 is skipped, its
 *      out_len bytes are the caller's to fill): the cleaned texts.  totals[0]: bytes written,
 *      totals[1]: lines whose text differs from out_len or does not fit (nothing is written there).
 * avdb_vep_output_update_write: avdb_vep_rows_update_write with the extra column, one wave per row:
 *   pk<TAB>chr<label><TAB>most severe<TAB>ranked<TAB>vep_output<TAB>alg_id[<TAB>true]<LF>
 * out_len: avdb_vep_rows_update_size's with 1 + len[row_entry[match]] added by the caller.  A row
 * whose parts do not add up to its out_len is left blank.
 * Workspace: avdb_vep_output_workspace_size (size, write), avdb_vep_rows_update_workspace_size
 * (update write). */
#define AVDB_VEPOUT_IDENTITY_ONLY 0x01u
#define AVDB_VEPOUT_N_REASONS 19
#define AVDB_VEPOUT_COUNT_LINES 0
#define AVDB_VEPOUT_COUNT_HOST_LINES 1
#define AVDB_VEPOUT_COUNT_OUT_BYTES 2
#define AVDB_VEPOUT_COUNT_REASON0 3
#define AVDB_VEPOUT_N_COUNTS 22
typedef struct avdb_vep_output_table {
  uint32_t struct_size; /* sizeof(avdb_vep_output_table) */
  uint32_t reserved;
  uint64_t n_entries;
  const uint8_t* text; /* the cleaned texts */
  uint64_t text_bytes;
  const uint64_t* off;      /* per entry */
  const uint32_t* len;      /* per entry */
  const int32_t* row_entry; /* per row of the avdb_vep_rows_table */
} avdb_vep_output_table;
int avdb_vep_output_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes);
int avdb_vep_output_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                         const avdb_vep_rows_in* in, const uint8_t* ent_flags, uint32_t flags, uint64_t* line_start,
                         uint32_t* out_len, uint32_t* dict_at, uint32_t* dict_len, uint8_t* out_flags, uint64_t* counts,
                         void* workspace, size_t workspace_bytes, void* stream);
int avdb_vep_output_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                          const avdb_vep_rows_in* in, uint32_t flags, const uint64_t* out_off, const uint32_t* out_len,
                          const uint32_t* dict_at, const uint32_t* dict_len, const uint8_t* out_flags, uint8_t* out,
                          size_t out_cap, uint64_t* totals, void* workspace, size_t workspace_bytes, void* stream);
int avdb_vep_output_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                              const avdb_vep_rows_in* in, const uint8_t* ent_flags, uint32_t flags,
                              uint64_t* line_start, uint32_t* out_len, uint32_t* dict_at, uint32_t* dict_len,
                              uint8_t* out_flags, uint64_t* counts);
int avdb_vep_output_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                               const avdb_vep_rows_in* in, uint32_t flags, const uint64_t* out_off,
                               const uint32_t* out_len, const uint32_t* dict_at, const uint32_t* dict_len,
                               const uint8_t* out_flags, uint8_t* out, size_t out_cap, uint64_t* totals);
int avdb_vep_output_update_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_rows,
                                 const avdb_vep_rows_table* table, const avdb_vep_output_table* cleaned, uint32_t flags,
                                 uint64_t alg_id, const uint64_t* row_start, const uint32_t* pk_len,
                                 const int32_t* match, const uint32_t* out_len, const uint8_t* row_flags, uint8_t* out,
                                 size_t out_cap, uint64_t* row_off, uint64_t* totals, void* workspace,
                                 size_t workspace_bytes, void* stream);
int avdb_vep_output_update_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                      size_t n_rows, const avdb_vep_rows_table* table,
                                      const avdb_vep_output_table* cleaned, uint32_t flags, uint64_t alg_id,
                                      const uint64_t* row_start, const uint32_t* pk_len, const int32_t* match,
                                      const uint32_t* out_len, const uint8_t* row_flags, uint8_t* out, size_t out_cap,
                                      uint64_t* row_off, uint64_t* totals);

/* ---- K18d: the allele_frequencies column of the VEP update rows --------------------------------
 * xstr(alleleFreq, nullStr='{}') of VEPVariantLoader.__parse_alt_alleles (vep_variant_loader.py:
 * 85-109, 126-142, 190-199), one text per ALT allele: VepJsonParser.get_frequencies' choice among
 * the elements of colocated_variants (one element: cv[0] when it has `frequencies`; more: the last
 * one whose allele_string is not COSMIC_MUTATION, that has `frequencies` and, with
 * AVDB_VEPFREQ_MATCH_REFSNP and a ref_snp_id in `input`, whose id is that), its `frequencies` of
 * the normalised ALT regrouped as {"GnomAD": {keys that hold gnomad}, "1000Genomes": {the others},
 * "ESP": {aa, ea}} (empty groups left out, members in source order), and the ALT's column of INFO
 * FREQ (not with AVDB_VEPFREQ_IDENTITY_ONLY) merged in: {"gmaf": x} inside the group a population
 * names, a new "pop": {"gmaf": x} behind the groups otherwise; '{}' when nothing is left.  On
 * K18a's arrays of the same slab (avdb_vep_rows_in; el_rlen is not read) and K18b's entries
 * (entry e is line e: ent_start its start, ent_alts its rows, row0 the sums of ent_alts before it).
 *   1. avdb_vep_freq_size: per line the span of the chosen `frequencies` object (fr_len 0: none),
 *      the span of FREQ's value (fq_len 0: none) and a flags byte: 0, or 1 + the reason the line is
 *      left to the caller; per table row the length of its text (0 for such a line).  Reasons: one
 *      of K18a or K18b (0 .. 15), 16 colocated_variants is no array, is empty or holds what is no
 *      object, 17 among several elements one without allele_string, or without id where one is
 *      matched, or either not a string, 18 a key of interest twice (colocated_variants; an element's
 *      allele_string, id, frequencies; the allele's key; a member's key), 19 a backslash or a byte
 *      outside printable ASCII inside colocated_variants, 20 `frequencies` or the allele's value is
 *      no object, 21 a member's value outside the token rule (avdb_vep_freq_token_ok_host), 22 more
 *      than AVDB_VEPFREQ_MAX_MEMBERS members, 23 a member named gmaf in a group FREQ names too, 24
 *      fewer than eight fields in `input`, a backslash other than the separators' or a byte < 0x20
 *      in them, an INFO to_numeric turns into a number, an RS to match that is not plain digits
 *      without a leading zero, 25 a FREQ avdb_vcf_format leaves to the host (no ':', more than 64
 *      or repeated populations, a name json.dumps escapes), a bare FREQ, '#' in its value, 26 a
 *      FREQ number that is not digits with at most one '.' and 15 significant digits, or fewer
 *      comma items than ALTs, 27 two ALTs with one normalised allele.  counts:
 *      AVDB_VEPFREQ_N_COUNTS x u64, set by the call.
 *   2. avdb_vep_freq_write (freq_off: the caller's offsets per row; a line with flags != 0 is
 *      skipped, its rows' bytes are the caller's to fill): the texts.  totals[0]: bytes written,
 *      totals[1]: rows whose text differs from freq_len or does not fit (nothing is written there).
 * avdb_vep_freq_update_write: avdb_vep_output_update_write with the column, one wave per row:
 *   pk<TAB>chr<label><TAB>allele_frequencies<TAB>most severe<TAB>ranked[<TAB>vep_output]<TAB>alg_id[<TAB>true]<LF>
 * cleaned: NULL for rows without vep_output.  out_len: avdb_vep_rows_update_size's with
 * 1 + len[match] (and 1 + the cleaned length) added by the caller.
 * Workspace: avdb_vep_freq_workspace_size (size), avdb_vep_rows_update_workspace_size (update write). */
#define AVDB_VEPFREQ_IDENTITY_ONLY 0x01u
#define AVDB_VEPFREQ_MATCH_REFSNP 0x02u
#define AVDB_VEPFREQ_MAX_MEMBERS 64
#define AVDB_VEPFREQ_N_REASONS 28
#define AVDB_VEPFREQ_COUNT_LINES 0
#define AVDB_VEPFREQ_COUNT_HOST_LINES 1
#define AVDB_VEPFREQ_COUNT_ROWS 2
#define AVDB_VEPFREQ_COUNT_OUT_BYTES 3
#define AVDB_VEPFREQ_COUNT_REASON0 4
#define AVDB_VEPFREQ_N_COUNTS 32
typedef struct avdb_vep_freq_table {
  uint32_t struct_size; /* sizeof(avdb_vep_freq_table) */
  uint32_t reserved;
  uint64_t n_rows;     /* the rows of the avdb_vep_rows_table */
  const uint8_t* text; /* the frequency texts */
  uint64_t text_bytes;
  const uint64_t* off; /* per row */
  const uint32_t* len; /* per row */
} avdb_vep_freq_table;
int avdb_vep_freq_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes);
int avdb_vep_freq_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_rows,
                       const avdb_vep_rows_in* in, const uint64_t* ent_start, const uint32_t* ent_alts,
                       const uint8_t* ent_flags, const uint64_t* row0, uint32_t flags, uint64_t* fr_start,
                       uint32_t* fr_len, uint64_t* fq_start, uint32_t* fq_len, uint8_t* out_flags, uint32_t* freq_len,
                       uint64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int avdb_vep_freq_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_rows,
                        const avdb_vep_rows_in* in, const uint32_t* ent_alts, const uint64_t* row0,
                        const uint64_t* fr_start, const uint32_t* fr_len, const uint64_t* fq_start,
                        const uint32_t* fq_len, const uint8_t* out_flags, const uint64_t* freq_off,
                        const uint32_t* freq_len, uint8_t* out, size_t out_cap, uint64_t* totals, void* workspace,
                        size_t workspace_bytes, void* stream);
int avdb_vep_freq_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_rows,
                            const avdb_vep_rows_in* in, const uint64_t* ent_start, const uint32_t* ent_alts,
                            const uint8_t* ent_flags, const uint64_t* row0, uint32_t flags, uint64_t* fr_start,
                            uint32_t* fr_len, uint64_t* fq_start, uint32_t* fq_len, uint8_t* out_flags,
                            uint32_t* freq_len, uint64_t* counts);
int avdb_vep_freq_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_rows,
                             const avdb_vep_rows_in* in, const uint32_t* ent_alts, const uint64_t* row0,
                             const uint64_t* fr_start, const uint32_t* fr_len, const uint64_t* fq_start,
                             const uint32_t* fq_len, const uint8_t* out_flags, const uint64_t* freq_off,
                             const uint32_t* freq_len, uint8_t* out, size_t out_cap, uint64_t* totals);
/* 1 when the n bytes are a value the device copies (reason 21's rule: avdb_vep_rows_token_ok_host's, or
 * D[.F]e-XX: D in 1 .. 9, F without a trailing zero, at most 15 significant digits, XX of two digits, or
 * three without a leading zero, its value in 5 .. 300), else 0 */
int avdb_vep_freq_token_ok_host(const uint8_t* token, size_t n);
int avdb_vep_freq_update_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_rows,
                               const avdb_vep_rows_table* table, const avdb_vep_freq_table* freq,
                               const avdb_vep_output_table* cleaned, uint32_t flags, uint64_t alg_id,
                               const uint64_t* row_start, const uint32_t* pk_len, const int32_t* match,
                               const uint32_t* out_len, const uint8_t* row_flags, uint8_t* out, size_t out_cap,
                               uint64_t* row_off, uint64_t* totals, void* workspace, size_t workspace_bytes,
                               void* stream);
int avdb_vep_freq_update_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                    size_t n_rows, const avdb_vep_rows_table* table, const avdb_vep_freq_table* freq,
                                    const avdb_vep_output_table* cleaned, uint32_t flags, uint64_t alg_id,
                                    const uint64_t* row_start, const uint32_t* pk_len, const int32_t* match,
                                    const uint32_t* out_len, const uint8_t* row_flags, uint8_t* out, size_t out_cap,
                                    uint64_t* row_off, uint64_t* totals);

/* ---- host-side formatting of kernel outputs -------------------------------
 * ltree path text (<= AVDB_MAX_PATH bytes).  Returns the length written (no
 * NUL terminator counted; one is written if cap allows), or a negative code. */
int avdb_format_bin_path(const avdb_ctx* ctx, uint8_t chrom, uint32_t bin_code, char* out_host,
                         size_t cap);
/* Batch form (host arrays): paths concatenated into out_host, out_off[i] the
 * start of path i, out_off[n] the total; returns AVDB_ERANGE if cap is short. */
int avdb_format_bin_paths(const avdb_ctx* ctx, const uint8_t* chrom_host, const uint32_t* code_host,
                          size_t n, char* out_host, size_t cap, uint64_t* out_off_host);

#ifdef __cplusplus
}
#endif
#endif /* AVDB_H_ */
