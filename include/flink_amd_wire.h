/*
 * flink_amd_wire.h -- on-GPU decoding of Flink's network wire format.
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
 * Supported value types: BIGINT / TIMESTAMP(p<=3) / TIMESTAMP_LTZ(p<=3) as FWA_FIELD_LONG, DOUBLE, FLOAT, INT, and
 * in ROWDATA rows CHAR / VARCHAR / STRING as FWA_FIELD_STRING (BinaryRowData's layout, AbstractBinaryWriter.java:
 * 80-105,279-334: a value of at most 7 bytes sits in its slot, top bit set and the length in the top byte; a longer
 * one in the row's variable-length part, slot = offset << 32 | length; the decoder follows each slot's own top bit
 * and does not assume that short values are inline). The bytes are handed on as they are, UTF-8 is not interpreted.
 * STRING fields come back through fwa_wire_strings_of in the layout fwa_key_strings takes, so a VARCHAR-keyed Table
 * job feeds fwa_keydict_encode from the channel's bytes without a host pass.
 *
 * Limits. An element (tag byte to its last byte; the 4-byte length prefix's value) may be at most 249 bytes: the
 * boundary maps keep entry offsets in a byte. A longer record ends the call with FWA_E_UNSUPPORTED and its byte
 * position, never FWA_E_CORRUPT; raising the ceiling needs 16-bit entry offsets in the maps and is a follow-up.
 * Not supported (FWA_E_UNSUPPORTED): STRING fields of TUPLE values (StringSerializer writes varint-prefixed UTF-16
 * code units, and DataStream String keys are FWA_KEY_PREHASHED), non-INSERT RowKinds, LZ4-compressed buffers
 * (taskmanager.network.compression), and the other variable-length SQL types (DECIMAL with p > 18, TIMESTAMP with
 * p > 3). Status codes: include/flink_amd.h.
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

/* Field types (java.lang.Long / BIGINT / compact TIMESTAMP, Double / DOUBLE, Float / FLOAT, Integer / INT, and
 * CHAR / VARCHAR / STRING of FWA_WIRE_ROWDATA rows). A STRING field cannot be key_field, ts_field or a col_field
 * (FWA_E_ARG); with FWA_WIRE_TUPLE it is FWA_E_UNSUPPORTED. */
enum fwa_wire_field { FWA_FIELD_LONG = 0, FWA_FIELD_DOUBLE = 1, FWA_FIELD_FLOAT = 2, FWA_FIELD_INT = 3, FWA_FIELD_STRING = 4 };

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
                                                FLOAT -> float (the input types fwa_push's aggregates read) */
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
    const void* col[FWA_MAX_COLS];           /* device [n_records] per value column */
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
 * that differs from the element's length, or a STRING slot pointing outside its row) returns
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

/* The values of STRING field `field` in the records of the last fwa_wire_decode, in record order: exactly what
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

#ifdef __cplusplus
}
#endif
#endif /* FLINK_AMD_WIRE_H */
