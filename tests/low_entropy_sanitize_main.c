/* Stand-alone driver for tests/test_low_entropy_grammar.py: the oracle's two low-entropy decoders over a file of streams, built with
 * -fsanitize=address,undefined on the CPU.  Every stream and every output buffer is a heap block of its exact size, so a read behind a
 * stream or a write behind an output is the sanitizer's to find.
 *
 * File: records of [u8 sectioned][u32 stream bytes][u32 expected return value][stream].  Exit status 0: every decoder returned what the
 * record expects; 1: one did not (the record's index is printed); anything else: the sanitizer's. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../oracle/hsrle_oracle.h"

int main(int argc, char **argv)
{
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;

  int bad = 0;
  uint32_t n = 0;
  for (;; n++)
  {
    uint8_t head[9];
    if (fread(head, 1, 9, f) != 9) break;
    uint32_t size, want;
    memcpy(&size, head + 1, 4);
    memcpy(&want, head + 5, 4);

    uint8_t *stream = (uint8_t *)malloc(size ? size : 1);
    if (size && fread(stream, 1, size, f) != size) return 2;

    uint32_t outSize = 0;
    if (size >= 8) memcpy(&outSize, stream + 4, 4);
    if (outSize > (1u << 26)) outSize = 1u << 26;
    uint8_t *out = (uint8_t *)malloc(outSize ? outSize : 1);

    const uint32_t got = head[0] ? hso_rle8m_decompress(stream, size, out, outSize) : hso_low_entropy_decompress(stream, size, out, outSize);
    if (got != want) { printf("record %u: returned %u, expected %u\n", n, got, want); bad = 1; }

    free(out);
    free(stream);
  }

  fclose(f);
  printf("%u records\n", n);
  return bad;
}
