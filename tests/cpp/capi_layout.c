/* What the C compiler makes of include/rvb_capi.h, one fact per line, for tests/test_capi_host.py to hold the Python mirrors against:
 *   sizeof <struct> <bytes>
 *   field <struct> <member> <offset> <bytes> <kind>     kind: f float, u unsigned integer, p pointer to float, s rvb_impulse
 *   value <macro or enumerator> <value>
 * The kind is not taken on trust: every line initialises a pointer to the kind's C type with the address of the member (of its first
 * element, for an array), which does not compile under -Werror when the header declares another type.  Plain C99, nothing but the header. */
#include <stddef.h>
#include <stdio.h>

#include "rvb_capi.h"

#define STRUCT(type) printf("sizeof " #type " %zu\n", sizeof(type))
#define FIELD(type, member, element, kind, ctype) do { \
        type object; \
        const ctype * same_type = &object.element; \
        (void) same_type; \
        printf("field " #type " " #member " %zu %zu " #kind "\n", offsetof(type, member), sizeof(object.member)); \
    } while (0)
#define FLOAT(type, member) FIELD(type, member, member, f, float)
#define FLOATS(type, member) FIELD(type, member, member[0], f, float)
#define U64(type, member) FIELD(type, member, member, u, uint64_t)
#define U32(type, member) FIELD(type, member, member, u, uint32_t)
#define VALUE(name) printf("value " #name " %ld\n", (long) (name))

int main(void) {
    STRUCT(rvb_triangle);
    U64(rvb_triangle, surface);
    U64(rvb_triangle, v0);
    U64(rvb_triangle, v1);
    U64(rvb_triangle, v2);
    STRUCT(rvb_float3);
    FLOATS(rvb_float3, s);
    STRUCT(rvb_surface);
    FLOATS(rvb_surface, specular);
    FLOATS(rvb_surface, diffuse);
    STRUCT(rvb_impulse);
    FLOATS(rvb_impulse, volume);
    FLOATS(rvb_impulse, position);
    FLOAT(rvb_impulse, time);
    FLOATS(rvb_impulse, pad_);
    STRUCT(rvb_attenuated_impulse);
    FLOATS(rvb_attenuated_impulse, volume);
    FLOAT(rvb_attenuated_impulse, time);
    FLOATS(rvb_attenuated_impulse, pad_);
    STRUCT(rvb_speaker);
    FLOATS(rvb_speaker, direction);
    FLOAT(rvb_speaker, coefficient);
    FLOATS(rvb_speaker, pad_);
    STRUCT(rvb_image_candidate);
    U64(rvb_image_candidate, ray);
    U32(rvb_image_candidate, slot);
    U32(rvb_image_candidate, index);
    FIELD(rvb_image_candidate, impulse, impulse, s, rvb_impulse);
    STRUCT(rvb_source_pattern);
    FLOATS(rvb_source_pattern, direction);
    FLOATS(rvb_source_pattern, shape);
    STRUCT(rvb_source_orientation);
    FLOATS(rvb_source_orientation, facing);
    FLOATS(rvb_source_orientation, up);
    STRUCT(rvb_pipeline_result);
    U64(rvb_pipeline_result, job);
    FIELD(rvb_pipeline_result, histogram, histogram, p, float * const);
    U64(rvb_pipeline_result, nchannels);
    U64(rvb_pipeline_result, nbins);
    FLOAT(rvb_pipeline_result, predelay);
    FLOAT(rvb_pipeline_result, max_time);
    U64(rvb_pipeline_result, nimages);
    STRUCT(rvb_pipeline_options);
    U64(rvb_pipeline_options, group);
    U64(rvb_pipeline_options, pairs_per_launch);

    VALUE(RVB_NUM_IMAGE_SOURCE);
    VALUE(RVB_NUM_BANDS);
    VALUE(RVB_OK);
    VALUE(RVB_ERR_INVALID);
    VALUE(RVB_ERR_NO_DEVICE);
    VALUE(RVB_ERR_HIP);
    VALUE(RVB_ERR_STATE);
    VALUE(RVB_ERR_CAPACITY);
    VALUE(RVB_IR_DIFFUSE);
    VALUE(RVB_IR_IMAGES);
    VALUE(RVB_IR_ALL);
    VALUE(RVB_IR_FAST);
    VALUE(RVB_IR_EXACT);
    VALUE(RVB_KEEP_MATERIALS);
    VALUE(RVB_KEEP_LISTENER);
    VALUE(RVB_DECAY_TILE);
    VALUE(RVB_DECAY_NORMALISED);
    VALUE(RVB_DECAY_EDT);
    VALUE(RVB_DECAY_T20);
    VALUE(RVB_DECAY_T30);
    VALUE(RVB_DECAY_C50);
    VALUE(RVB_DECAY_C80);
    VALUE(RVB_DECAY_D50);
    VALUE(RVB_DECAY_TS);
    VALUE(RVB_DECAY_NPARAMS);
    VALUE(RVB_GRAD_MAP_TILE);
    VALUE(RVB_MAX_SPEAKERS);
    VALUE(RVB_PIPELINE_MAX_PAIRS);
    VALUE(RVB_MULTI_REHEARSE_RCCL);
    return 0;
}
