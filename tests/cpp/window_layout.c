/* What the C compiler makes of include/rvb_capi_window.h, one fact per line, for tests/test_window_header_host.py to hold the numpy
 * dtypes and constants of capi.py against (the format of tests/cpp/capi_layout.c):
 *   sizeof <struct> <bytes>
 *   field <struct> <member> <offset> <bytes> <kind>     kind: f float, u unsigned integer
 *   value <macro> <value>
 * Every line initialises a pointer to the kind's C type with the address of the member (of its first element, for an array), which does
 * not compile under -Werror when the header declares another type.  Plain C99, nothing but the header. */
#include <stddef.h>
#include <stdio.h>

#include "rvb_capi_window.h"

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
    STRUCT(rvb_window_entry);
    U64(rvb_window_entry, record);
    FLOAT(rvb_window_entry, score);
    FLOAT(rvb_window_entry, time);
    STRUCT(rvb_window_path);
    U64(rvb_window_path, ray);
    U32(rvb_window_path, bounce);
    U32(rvb_window_path, nhits);
    FLOAT(rvb_window_path, score);
    FLOAT(rvb_window_path, time);
    FLOATS(rvb_window_path, pad_);
    FLOATS(rvb_window_path, volume);
    STRUCT(rvb_window_hit);
    FLOATS(rvb_window_hit, position);
    U32(rvb_window_hit, triangle);

    VALUE(RVB_WINDOW_TILE);
    VALUE(RVB_WINDOW_MAX_PATHS);
    return 0;
}
