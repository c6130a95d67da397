/*
 * flink_amd_wire.h -- on-GPU decoding of Flink's network wire format, and, in the second
 * half of this header, its encoding (fwa_wire_encode: fired rows written as channel bytes).
 *
 * Upstream of the window operator, Flink's StreamTask input deserialises every StreamElement of a channel
 * from its network buffers on the task thread, one virtual call chain per record:
 *   SpillingAdaptiveSpanningRecordDeserializer.getNextRecord  (.../io/network/api/serialization/
 *     SpillingAdaptiveSpanningRecordDeserializer.java:88-131: a 4-byte big-endian length, then the
 *     element; an element may span buffers, SpanningWrapper)
 *   -> StreamElementSerializer.deserialize  (flink-streaming-java/.../streamrecord/StreamElementSerializer.java:
 *     tag byte :48-53, then TAG_REC_WITH_TIMESTAMP: long ts + value, TAG_REC_WITHOUT_TIMESTAMP: value,
 *     TAG_WATERMARK: long, TAG_STREAM_STATUS: int, TAG_LATENCY_MARKER: long, long, long, int,
 *     TAG_RECORD_ATTRIBUTES: boolean -- :190-211; written by serialize :158-187 behind
 *     RecordWriter.serializeRecord's length prefix, RecordWriter.java:145-157)
 *   -> the value serializer: TupleSerializer of Long/Double/Float/Integer fields (java.io.DataOutput
 *     big-endian), or RowDataSerializer -> BinaryRowDataSerializer.serialize (BinaryRowDataSerializer.java:
 *     85-93: int size, then the BinaryRowData bytes: null bit set with the RowKind in byte 0, 8-byte
 *     little-endian fixed-length slots, BinaryRowData.java:68-75,114-116)
 *   -> AbstractStreamTaskNetworkInput.processElement (:154-181) dispatches records to the operator and
 *     watermarks / status / latency markers / record attributes to their handlers.
 *
 * fwa_wire_decode replaces that loop for the records of one input channel: the channel's data-buffer
 * payloads, concatenated in arrival order, are parsed on the GPU into the SoA columns fwa_push takes
 * (FWA_PUSH_DEVICE_PTRS, zero copy), and the non-record elements come back as an ordered event list
 * carrying the record position they sit at, so the caller interleaves fwa_push / fwa_advance_watermark
 * exactly as processElement would. Element boundaries are found on the GPU (every chunk parses all its
 * candidate entry offsets; the chunk maps are composed hierarchically), so no host pass touches the bytes.
 *
 * Supported value types: BIGINT / TIMESTAMP(p<=3) / TIMESTAMP_LTZ(p<=3) / DECIMAL(p<=18) as FWA_FIELD_LONG (a compact
 * DECIMAL is its unscaled long in the 8-byte slot, AbstractBinaryWriter.writeDecimal :164-171), DOUBLE, FLOAT, INT, and
 * in ROWDATA rows CHAR / VARCHAR / STRING as FWA_FIELD_STRING (BinaryRowData's layout, AbstractBinaryWriter.java:
 * 80-105,279-334: a value of at most 7 bytes sits in its slot, top bit set and the length in the top byte; a longer
 * one in the row's variable-length part, slot = offset << 32 | length; the decoder follows each slot's own top bit
 * and does not assume that short values are inline). The bytes are handed on as they are, UTF-8 is not interpreted.
 * STRING fields come back through fwa_wire_strings_of in the layout fwa_key_strings takes, so a VARCHAR-keyed Table
 * job feeds fwa_keydict_encode from the channel's bytes without a host pass.
 * In ROWDATA rows a DECIMAL with precision > 18 is FWA_FIELD_DECIMAL (non-compact, AbstractBinaryWriter.writeDecimal
 * :164-196, read back by BinarySegmentUtils.readDecimalData -> DecimalData.fromUnscaledBytes -> new BigInteger(bytes)):
 * 16 bytes are reserved at the writer's cursor in the row's variable-length part and zeroed,
 * DecimalData.toUnscaledBytes() (BigInteger.toByteArray: the minimal big-endian two's complement, bitLength / 8 + 1 =
 * 1..16 bytes) is copied to their start, the slot is offset << 32 | length with the offset counted from the row's first
 * byte, and the cursor advances by 16 whatever the length; the variable-length parts follow the fixed part in field
 * order, interleaved with the 8-rounded parts of long STRING values. A NULL DECIMAL has two forms on the wire:
 * RowDataSerializer.toBinaryRow (:196-212, the form the window operator's JoinedRowData output goes through) calls
 * setNullAt -- the null bit, a zero slot, nothing reserved -- while a row built directly by a BinaryRowWriter may come
 * from writeDecimal(pos, null, precision) -- the null bit, slot = cursor << 32 | 0, 16 zero bytes reserved. The decoder
 * accepts both (it reads the null bit first and never interprets the slot of a NULL field); the encoder writes the
 * first. A decoded DECIMAL column is 16-byte little-endian two's complement values, the input of FWA_SUM_DEC128 /
 * FWA_AVG_DEC128; the 38-digit bound is theirs to apply, not the decoder's.
 *
 * In TUPLE values a java.lang.String field is FWA_FIELD_JSTRING (StringSerializer.serialize -> StringValue.writeString,
 * read back by StringValue.readString; flink-core/.../types/StringValue.java): len + 1 in 7-bit groups, low group first,
 * every group but the last with bit 7 set (len = the number of UTF-16 code units), then each code unit coded the same
 * way -- 1 to 3 bytes, a third byte at most 0x03. A null String is the single byte 00. Nothing is aligned or padded:
 * the fields behind a String start where it ended. "key1" is 05 6b 65 79 31, "" is 01, U+FFFF is 02 ff ff 03.
 * The canonical form of a value is its char bytes exactly as they stand on the wire (the bytes behind the length
 * prefix): that is what fwa_wire_strings_of returns, what the key dictionary stores and what the encoder writes back
 * behind a new prefix. For ASCII it is the text itself. Every Flink writer produces the shortest coding of a char, so
 * two Strings are equal iff these bytes are equal (the dictionary's byte equality needs exactly that), the code-unit
 * count is the number of bytes below 0x80, nothing is transcoded in either direction and lone surrogates survive.
 * A key dictionary must not mix these values with UTF-8 FWA_FIELD_STRING values: the same non-ASCII text has different
 * bytes in the two forms. Stated deviation: the reference reader accepts a non-canonical char (more than 3 groups, a
 * value above 0xFFFF, a multi-byte char whose last group is zero) and truncates it with (char); the decoder answers
 * FWA_E_CORRUPT, since no writer produces such bytes and accepting them would make byte equality differ from String
 * equality. A length prefix of several groups whose value is 0 (80 00; the reference reader would ask for a char[-1])
 * is FWA_E_CORRUPT as well. A schema with a JSTRING field has key_field -1; a DataStream String key goes to a
 * FWA_KEY_PREHASHED handle as fwa_keydict_encode ids beside fwa_jstring_hash hashes, both computed on the device.
 *
 * Limits. An element (tag byte to its last byte; the 4-byte length prefix's value) may be at most 249 bytes: the
 * boundary maps keep entry offsets in a byte. A longer record ends the call with FWA_E_UNSUPPORTED and its byte
 * position, never FWA_E_CORRUPT; raising the ceiling needs 16-bit entry offsets in the maps and is a follow-up.
 * Not supported (FWA_E_UNSUPPORTED): FWA_FIELD_STRING in TUPLE values (a Tuple's String is FWA_FIELD_JSTRING) and
 * FWA_FIELD_JSTRING in ROWDATA rows, String fields as value columns or as key_field, non-INSERT RowKinds, LZ4-compressed buffers
 * (taskmanager.network.compression), DECIMAL fields of TUPLE values (BigDecSerializer is another format) or as key
 * dictionary columns, and the other variable-length SQL types (TIMESTAMP with p > 3). Status codes:
 * include/flink_amd.h.
 */
#ifndef FLINK_AMD_WIRE_H
#define FLINK_AMD_WIRE_H

#include <stdint.h>

#include "flink_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FWA_WIRE_MAX_FIELDS 16

/* StreamElementSerializer tags (StreamElementSerializer.java:48-53) */
enum fwa_wire_tag {
    FWA_TAG_REC_WITH_TIMESTAMP = 0,
    FWA_TAG_REC_WITHOUT_TIMESTAMP = 1,
    FWA_TAG_WATERMARK = 2,
    FWA_TAG_LATENCY_MARKER = 3,
    FWA_TAG_STREAM_STATUS = 4,
    FWA_TAG_RECORD_ATTRIBUTES = 5
};

/* Value serializer of the channel's StreamRecords. */
enum fwa_wire_format {
    FWA_WIRE_TUPLE = 0,    /* TupleSerializer (DataStream Tuple2..Tuple16): fields back to back, big-endian
                              (LongSerializer / DoubleSerializer / FloatSerializer / IntSerializer) */
    FWA_WIRE_ROWDATA = 1   /* RowDataSerializer -> BinaryRowDataSerializer (Table runtime rows) */
};

/* Field types (java.lang.Long / BIGINT / compact TIMESTAMP / compact DECIMAL, Double / DOUBLE, Float / FLOAT, Integer /
 * INT, and in FWA_WIRE_ROWDATA rows CHAR / VARCHAR / STRING and DECIMAL(p > 18)). A STRING field cannot be key_field,
 * ts_field or a col_field (FWA_E_ARG); with FWA_WIRE_TUPLE it is FWA_E_UNSUPPORTED. A DECIMAL field may be a col_field
 * (or be read by no column: it is skipped); as key_field or ts_field it is FWA_E_ARG, with FWA_WIRE_TUPLE
 * FWA_E_UNSUPPORTED. Value 5 is unassigned and stays refused (FWA_E_UNSUPPORTED by the decoder, FWA_E_ARG by the
 * encoder), like every other unknown value, and so does 7. A JSTRING field (java.lang.String of a FWA_WIRE_TUPLE value;
 * any number of them, at any position) cannot be key_field, ts_field or a col_field (FWA_E_ARG), its schema has
 * key_field -1 (FWA_E_ARG otherwise; batch.key / key_null are NULL), and with FWA_WIRE_ROWDATA it is FWA_E_UNSUPPORTED. */
enum fwa_wire_field {
    FWA_FIELD_LONG = 0, FWA_FIELD_DOUBLE = 1, FWA_FIELD_FLOAT = 2, FWA_FIELD_INT = 3, FWA_FIELD_STRING = 4,
    FWA_FIELD_DECIMAL = 6, FWA_FIELD_JSTRING = 8
};

typedef struct fwa_wire_schema {
    int32_t format;                          /* enum fwa_wire_format */
    int32_t arity;                           /* fields per value, 1..FWA_WIRE_MAX_FIELDS */
    int32_t field[FWA_WIRE_MAX_FIELDS];      /* enum fwa_wire_field of each field */
    int32_t key_field;                       /* field -> key column (int64; INT sign-extended). -1 in a schema with
                                                a STRING field: the caller builds the key from string fields and
                                                columns (fwa_keydict_encode); batch.key / key_null are then NULL */
    int32_t ts_field;                        /* field -> ts column; -1: the StreamRecord timestamp (records
                                                written without one get INT64_MIN, StreamRecord.hasTimestamp
                                                false, which fwa_push rejects with FWA_E_TS_MIN like
                                                TumblingEventTimeWindows.java:83-86) */
    int32_t num_cols;                        /* value columns */
    int32_t col_field[FWA_MAX_COLS];         /* field -> value column c: LONG/INT -> int64, DOUBLE -> double,
                                                FLOAT -> float (the input types fwa_push's aggregates read);
                                                DECIMAL -> 16-byte little-endian two's complement (low 8 bytes, then
                                                high), 16-byte aligned: the input of FWA_SUM_DEC128 / FWA_AVG_DEC128 */
    int32_t device;                          /* HIP device ordinal */
    int64_t max_bytes;                       /* sizing hint: largest nbytes per call (0 = 64 MiB; grows) */
} fwa_wire_schema;

typedef struct fwa_wire_decoder fwa_wire_decoder;

/* One decoded span of a channel. Device columns are decoder-owned and valid until the next call on it. */
typedef struct fwa_wire_batch {
    int64_t n_records;                       /* StreamRecords decoded, in stream order */
    int64_t n_events;                        /* non-record elements decoded */
    int64_t consumed;                        /* bytes of whole elements; [consumed, nbytes) is the head of an
                                                element continuing in the next buffer (SpanningWrapper): pass
                                                those bytes first in the next call */
    const int64_t* key;                      /* device [n_records] */
    const int64_t* ts;                       /* device [n_records] */
    const void* col[FWA_MAX_COLS];           /* device [n_records] per value column (a NULL DECIMAL field is 0) */
    const uint8_t* col_null[FWA_MAX_COLS];   /* ROWDATA: device [n_records], 1 = the field is NULL (the row's
                                                null bit; fwa_push_nullable's null_cols); NULL for TUPLE */
    const uint8_t* key_null;                 /* ROWDATA: device [n_records], 1 = NULL key field */
    /* events, host memory, in stream order */
    const int64_t* evt_pos;                  /* records of this batch that precede the event */
    const int32_t* evt_tag;                  /* enum fwa_wire_tag (2..5) */
    const int64_t* evt_val;                  /* [4 * n_events]: WATERMARK {timestamp}; STREAM_STATUS {status};
                                                LATENCY_MARKER {markedTime, operatorId.lower, operatorId.upper,
                                                subtaskIndex}; RECORD_ATTRIBUTES {isBacklog} */
} fwa_wire_batch;

/* Input location flag (same value as FWA_PUSH_DEVICE_PTRS): bytes is a device (HBM) pointer. */
#define FWA_WIRE_DEVICE_BYTES 0x1

int fwa_wire_create(const fwa_wire_schema* schema, fwa_wire_decoder** out);
void fwa_wire_destroy(fwa_wire_decoder* d);
const char* fwa_wire_last_error(const fwa_wire_decoder* d);

/* Decode the elements of bytes[0, nbytes) (concatenated buffer payloads of one channel, starting at an
 * element boundary). Device bytes (FWA_WIRE_DEVICE_BYTES) must be complete when the call is made: the decoder
 * runs on its own stream (the caller synchronises the producer's stream first); everything is complete on
 * return. A malformed element (unknown tag, a length that does not match its tag and the schema, a row size int
 * that differs from the element's length, a STRING slot pointing outside its row, a TUPLE value with JSTRING fields
 * whose field walk does not end exactly at the element's end or meets a non-canonical char, or the slot of a non-NULL DECIMAL
 * column whose bytes lie outside the row's variable-length part or number 0 or more than 16) returns
 * FWA_E_CORRUPT ("Corrupt stream, found tag", StreamElementSerializer.java:208-210).
 * Device timing of the decode kernels accumulates in fwa_wire_stats. */
int fwa_wire_decode(fwa_wire_decoder* d, const uint8_t* bytes, int64_t nbytes, int32_t flags,
                    fwa_wire_batch* out);

typedef struct fwa_wire_stats {
    int64_t calls;
    int64_t bytes_in;
    int64_t records_out;
    double decode_ms;                        /* HIP-event device time of the decode kernels */
    double scan_ms;                          /* of which: the chunk-map pass (boundary candidates) */
} fwa_wire_stats;

int fwa_wire_get_stats(fwa_wire_decoder* d, fwa_wire_stats* out);

/* The values of STRING or JSTRING field `field` (a JSTRING's canonical char bytes) in the records of the last fwa_wire_decode, in record order: exactly what
 * fwa_key_strings takes ({offsets + a, bytes} are records [a, b) for fwa_keydict_encode, no copy). Decoder-owned,
 * valid until the next call of fwa_wire_decode on it. A NULL field has length 0 and null = 1.
 * The extraction is lazy (a device scan of the lengths, then a gather from the wire bytes), so those bytes must
 * still be resident: host input lives in the decoder's staging buffer; with FWA_WIRE_DEVICE_BYTES the caller's
 * buffer must stay valid and unchanged until the strings of every field it wants have been fetched, or the next
 * decode begins. FWA_E_ARG: not a STRING field; FWA_E_STATE: no successful decode before it; FWA_E_UNSUPPORTED: the
 * field's bytes of one decode reach 2^31 (int32 offsets). */
typedef struct fwa_wire_strings {
    const int32_t* offsets;                  /* device [n_records + 1], offsets[0] = 0 */
    const uint8_t* bytes;                    /* device [offsets[n_records]] */
    const uint8_t* null;                     /* device [n_records], 1 = NULL */
    int64_t total_bytes;
} fwa_wire_strings;
int fwa_wire_strings_of(fwa_wire_decoder* d, int32_t field, fwa_wire_strings* out);

/* String.hashCode() (s[0]*31^(n-1) + ... + s[n-1] over UTF-16 code units, int wrap-around) of n values in the
 * canonical char-byte form, device pointers, Arrow offsets that need not start at 0; nulls may be NULL; a NULL
 * value hashes to 0. The key_hash column of fwa_push for FWA_KEY_PREHASHED; the counterpart of fwa_binrow_hash.
 * Runs on the device's default stream and is complete on return. */
int fwa_jstring_hash(const int32_t* offsets, const uint8_t* bytes, const uint8_t* nulls, int64_t n,
                     int32_t* out, int32_t device);

/* ---- wire encoder: fired rows written as channel bytes on the GPU ----
 *
 * Downstream of the window operator, Flink's task thread sends every fired row through one virtual call chain:
 *   RecordWriterOutput.collect -> pushToRecordWriter  (flink-streaming-java/.../runtime/io/RecordWriterOutput.java:
 *     131-135: the SerializationDelegate around the StreamRecord)
 *   -> RecordWriter.emit / serializeRecord  (flink-runtime/.../io/network/api/writer/RecordWriter.java:104-157: four
 *     bytes are skipped, the element is written, the 4-byte big-endian length is put in front; the bytes are then
 *     copied into the target subpartition's buffers, an element spanning buffers freely)
 *   -> StreamElementSerializer.serialize  (StreamElementSerializer.java:158-187: tag byte, [long timestamp], value;
 *     watermark, status, latency marker and record attributes with the payloads listed at fwa_wire_batch.evt_val)
 *   -> the value serializer: TupleSerializer (big-endian fields back to back), or RowDataSerializer ->
 *     BinaryRowDataSerializer.serialize (BinaryRowDataSerializer.java:85-93: int size, then the row's bytes as
 *     BinaryRowWriter laid them out, AbstractBinaryWriter.java:80-105,279-334: RowKind in byte 0, the null bit of
 *     field i at bit i + 8, 8-byte little-endian slots, INT / FLOAT in the low half of a zeroed slot, setNullAt
 *     zeroing the slot, a STRING of at most 7 bytes in its slot with 0x80 | length in the top byte, a longer one in
 *     the variable-length part, zero-padded to 8 bytes, slot = offset << 32 | length, a non-compact DECIMAL as laid
 *     out at the top of this header: :164-196).
 * fwa_wire_encode replaces that loop for the rows of one watermark step: the SoA columns fwa_advance_watermark returns
 * (fwa_out), and for a dictionary-keyed Table job the key columns fwa_keydict_decode returns, become the bytes
 *   be32 L | tag | [be64 ts] | value          per row, in row order, followed by the non-record elements given
 * in HBM, byte for byte what the chain above writes. A watermark step is "rows, then the watermark"
 * (AbstractStreamOperator.processWatermark :610-615). Cutting the bytes into 32 KiB network buffers stays with the
 * caller; elements span buffers freely. The GPU decoder above is a receiver of these bytes.
 *
 * Limits. arity 1..FWA_WIRE_MAX_FIELDS; KEYCOL index < FWA_KEYDICT_MAX_ARITY; STRING fields in ROWDATA rows only and
 * JSTRING fields in TUPLE values only (FWA_E_ARG). A JSTRING field takes one source, a FWA_SRC_KEYCOL column of type
 * FWA_KEY_FIELD_STRING holding values in the canonical char-byte form (the dictionary-decoded keys of a job fed by the
 * decoder above): the varint of (count of bytes below 0x80) + 1, then the bytes verbatim, the fields behind it
 * unaligned; a TUPLE value cannot carry NULLs (FWA_E_ARG at encode when a source has NULL flags). The DECIMAL
 * aggregates (FWA_SUM_DEC / FWA_AVG_DEC / FWA_SUM_DEC128 / FWA_AVG_DEC128: every result is a DECIMAL(38, s), 16 bytes
 * per row in fwa_out) are written as FWA_FIELD_DECIMAL only, in ROWDATA rows: the minimal unscaled bytes in 16 reserved
 * ones, a NULL result (agg_null) as setNullAt, the form RowDataSerializer.toBinaryRow :196-212 gives the operator's
 * output rows. Under any other wire type they are FWA_E_UNSUPPORTED, and a FWA_FIELD_DECIMAL field takes no other
 * source (FWA_E_ARG); a BigDecimal field of a TUPLE value (BigDecSerializer) is not written (FWA_E_ARG). Not supported:
 * TIMESTAMP with p > 3. The decoder's 249-byte element ceiling does not apply: element offsets are 64-bit, and a STRING
 * value may be as long as its int32 Arrow offsets allow. */

/* Where a field's value comes from. */
enum fwa_wire_src {
    FWA_SRC_KEY = 0,        /* fwa_out.key                                                    (int64) */
    FWA_SRC_KEYCOL = 1,     /* column src_index of fwa_wire_keycols (the decoded key dictionary row) */
    FWA_SRC_WIN_START = 2,  /* fwa_out.win_start, as the engine returns it                    (int64) */
    FWA_SRC_WIN_END = 3,    /* fwa_out.win_end, as the engine returns it                      (int64) */
    FWA_SRC_WIN_TIME = 4,   /* win_end - 1: the window_time / TimeWindow.maxTimestamp column  (int64) */
    FWA_SRC_AGG = 5         /* fwa_out.agg[src_index], NULL where fwa_out.agg_null[src_index] says so */
};
enum fwa_wire_record_ts {
    FWA_REC_TS_NONE = 0,    /* TAG_REC_WITHOUT_TIMESTAMP (Table rows) */
    FWA_REC_TS_WIN_TIME = 1 /* TAG_REC_WITH_TIMESTAMP, win_end - 1 (WindowOperator.emitWindowContents :552-557) */
};

/* The rows' layout on the wire. The field order is the caller's: a Table window TVF row is key fields, aggregates,
 * window_start, window_end (AbstractWindowAggProcessor.collect :230-233); a legacy GROUP BY SESSION row orders its
 * window properties as the query does.
 * Allowed source -> wire type pairs (anything else is FWA_E_ARG at create): an int64 column -> LONG, or INT (the low
 * 32 bits, Java's narrowing cast); an int32 column -> INT, or LONG (sign-extended); double -> DOUBLE; float -> FLOAT;
 * a key dictionary STRING column -> STRING (ROWDATA) or JSTRING (TUPLE); a DECIMAL aggregate (FWA_SRC_AGG with src_kind FWA_SUM_DEC .. FWA_AVG_DEC128,
 * 14..17) -> DECIMAL and nothing else. FWA_FIRST_64 / FWA_SEL_64 hold a field's raw bits and also go out as DOUBLE,
 * FWA_FIRST_32 / FWA_SEL_32 also as FLOAT. */
typedef struct fwa_wire_out_schema {
    int32_t format;                          /* enum fwa_wire_format */
    int32_t arity;                           /* fields per value, 1..FWA_WIRE_MAX_FIELDS */
    int32_t field[FWA_WIRE_MAX_FIELDS];      /* enum fwa_wire_field: the wire type of each field */
    int32_t src[FWA_WIRE_MAX_FIELDS];        /* enum fwa_wire_src */
    int32_t src_index[FWA_WIRE_MAX_FIELDS];  /* FWA_SRC_AGG: aggregate j (0..FWA_MAX_AGGS-1); FWA_SRC_KEYCOL: column k
                                                (0..FWA_KEYDICT_MAX_ARITY-1); ignored otherwise */
    int32_t src_kind[FWA_WIRE_MAX_FIELDS];   /* the result dtype of a column is not visible in fwa_out, so the schema
                                                names it. FWA_SRC_AGG: the aggregate's fwa_agg_spec.kind (FWA_AGG_DISTINCT
                                                bit allowed), which fixes its result column: [i64], [i32], [f64] or
                                                [f32] as listed at enum fwa_agg_kind, or the 16-byte DECIMAL results.
                                                FWA_SRC_KEYCOL: the column's enum
                                                fwa_key_field_type. Ignored otherwise */
    int32_t record_ts;                       /* enum fwa_wire_record_ts */
    int32_t device;                          /* HIP device ordinal */
    int64_t max_bytes;                       /* sizing hint: largest output per call (0 = 64 MiB; grows) */
} fwa_wire_out_schema;

/* The decoded key dictionary rows of the fired ids (fwa_keydict_decode on fwa_out.key), row i beside row i of the
 * fwa_out. Always DEVICE pointers, also when the rows are host memory. */
typedef struct fwa_wire_keycols {
    int32_t n_cols;                                  /* columns given, <= FWA_KEYDICT_MAX_ARITY */
    int32_t pad;
    const void* col[FWA_KEYDICT_MAX_ARITY];          /* BIGINT int64 / INT int32 / DOUBLE double [n_rows]; unused for STRING */
    const uint8_t* null[FWA_KEYDICT_MAX_ARITY];      /* [n_rows], 1 = NULL; NULL pointer = no NULLs in the column */
    fwa_key_strings str[FWA_KEYDICT_MAX_ARITY];      /* STRING column: offsets [n_rows + 1] (need not start at 0), bytes;
                                                        a NULL value's bytes are not read */
} fwa_wire_keycols;

/* A non-record element: tag 2..5 and the payload of fwa_wire_batch.evt_val. */
typedef struct fwa_wire_event {
    int32_t tag;                             /* enum fwa_wire_tag, FWA_TAG_WATERMARK..FWA_TAG_RECORD_ATTRIBUTES */
    int32_t pad;
    int64_t val[4];
} fwa_wire_event;

typedef struct fwa_wire_bytes {
    const uint8_t* dev;                      /* device [nbytes], encoder-owned, valid until the next call on it */
    const uint8_t* host;                     /* with FWA_WIRE_HOST_BYTES: a host copy (pinned, encoder-owned, valid as
                                                long); NULL otherwise */
    int64_t nbytes;
} fwa_wire_bytes;

/* fwa_wire_encode flag: also copy the bytes to host memory (a shim handing them to JVM network buffers). */
#define FWA_WIRE_HOST_BYTES 0x2

typedef struct fwa_wire_encoder fwa_wire_encoder;

/* FWA_E_ARG: unknown format / field / source, arity or an index out of range, STRING or DECIMAL in a TUPLE value,
 * JSTRING in a ROWDATA row or over any source but a key dictionary STRING column, a
 * source -> wire type pair that is not allowed. FWA_E_UNSUPPORTED: a DECIMAL aggregate source under a wire type other
 * than FWA_FIELD_DECIMAL. FWA_E_DEVICE / FWA_E_OOM: HIP.
 * fwa_wire_enc_last_error(NULL) says why a create failed (per thread). */
int fwa_wire_enc_create(const fwa_wire_out_schema* schema, fwa_wire_encoder** out);
void fwa_wire_enc_destroy(fwa_wire_encoder* e);
const char* fwa_wire_enc_last_error(const fwa_wire_encoder* e);

/* Row i of `rows` becomes element i; the n_events non-record elements follow the rows, in order (zero rows with events
 * is legal, and so is neither: 0 bytes). rows->on_device == 0: the columns the schema reads are staged through the
 * encoder, as the decoder stages host bytes. Device columns must be complete when the call is made (the encoder runs
 * on its own stream); everything, the host copy included, is complete on return. keycols may be NULL when no field is
 * FWA_SRC_KEYCOL.
 * FWA_E_ARG: a column the schema reads is missing (KEYCOL without keycols / past n_cols, an aggregate past
 * rows->num_aggs, a NULL pointer with n_rows > 0), an event tag outside 2..5, or a TUPLE schema whose source has NULL
 * flags (a non-NULL agg_null / keycols->null pointer: TupleSerializer cannot write null fields).
 * Device timing accumulates in fwa_wire_enc_stats. */
int fwa_wire_encode(fwa_wire_encoder* e, const fwa_out* rows, const fwa_wire_keycols* keycols,
                    const fwa_wire_event* events, int32_t n_events, int32_t flags, fwa_wire_bytes* out);

typedef struct fwa_wire_enc_stats {
    int64_t calls;
    int64_t rows_in;
    int64_t bytes_out;
    double encode_ms;                        /* HIP-event device time of the encode kernels (size + scan + write) */
    double scan_ms;                          /* of which: the exclusive scan to element offsets (STRING / DECIMAL schemas) */
    double size_ms;                          /* of which: the size pass (STRING / DECIMAL schemas) */
} fwa_wire_enc_stats;

int fwa_wire_enc_get_stats(fwa_wire_encoder* e, fwa_wire_enc_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* FLINK_AMD_WIRE_H */
