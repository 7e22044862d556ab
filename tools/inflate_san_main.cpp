// inflate_san_main.cpp — a stand-alone program over the inflate of factor columns for sanitizer builds: the shared routine
// (lrf_amd/csrc/lrf_inflate_shared.h) through lrf_pack.cpp's entry lrf_pack_inflate_column_i8, on every stream of the file
// tests/inflate_cases.py dumps (the corpus, the hand-built streams and CORRUPT).  Each stream is copied into a heap block of
// exactly its length and inflated into a heap block of exactly its elements, at strides 1 and 3, so that a read or a write one
// byte outside either is an AddressSanitizer report.
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -o inflate_san tools/inflate_san_main.cpp -lz
//   ./inflate_san streams.bin
// File: int64 count; per stream int64 rows, int64 length, int64 ok, the stream, and when ok the `rows` bytes it inflates to.
#include "../lrf_amd/csrc/lrf_pack.cpp"

#include <cstdint>
#include <cstdio>
#include <vector>

static bool read_i64(FILE* f, int64_t* v) { return fread(v, sizeof(*v), 1, f) == 1; }

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s streams.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t count = 0, bad = 0;
    if (!read_i64(f, &count)) return 2;
    for (int64_t i = 0; i < count; i++) {
        int64_t rows, len, ok;
        if (!read_i64(f, &rows) || !read_i64(f, &len) || !read_i64(f, &ok) || rows < 1 || len < 0) { fprintf(stderr, "stream %ld: bad record\n", (long)i); return 2; }
        uint8_t* src = new uint8_t[(size_t)len ? (size_t)len : 1]; // (a block of its own: the redzone starts right behind the stream)
        std::vector<int8_t> want((size_t)(ok ? rows : 0));
        if ((len && fread(src, 1, (size_t)len, f) != (size_t)len) || (ok && fread(want.data(), 1, (size_t)rows, f) != (size_t)rows)) return 2;
        uint8_t* exact = len ? new uint8_t[(size_t)len] : nullptr;
        if (len) memcpy(exact, src, (size_t)len);
        for (int64_t stride : {(int64_t)1, (int64_t)3}) {
            const size_t elems = (size_t)((rows - 1) * stride + 1); // the last element is the block's last byte
            int8_t* dst = new int8_t[elems];
            memset(dst, 0x5A, elems);
            const int rc = lrf_pack_inflate_column_i8(len ? exact : src, len, dst, rows, stride);
            if ((rc == 0) != (ok != 0)) { fprintf(stderr, "stream %ld stride %ld: status %d, expected %s\n", (long)i, (long)stride, rc, ok ? "0" : "a refusal"); bad++; }
            if (rc == 0 && ok)
                for (int64_t r = 0; r < rows; r++)
                    if (dst[r * stride] != want[(size_t)r]) { fprintf(stderr, "stream %ld stride %ld: byte %ld differs\n", (long)i, (long)stride, (long)r); bad++; break; }
            for (size_t e = 0; e < elems; e++)
                if (e % (size_t)stride && dst[e] != 0x5A) { fprintf(stderr, "stream %ld stride %ld: padding %zu written\n", (long)i, (long)stride, e); bad++; break; }
            delete[] dst;
        }
        delete[] exact;
        delete[] src;
    }
    fclose(f);
    printf("%ld streams, %ld failures\n", (long)count, (long)bad);
    return bad ? 1 : 0;
}
