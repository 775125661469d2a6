// 48 bit symbols: rle48_{sym,byte}[_packed], rle48_{3,7}symlut_{sym,byte}  (reference: src/rle.h)
#define HSRLE_S 6
#include "hsrle_inst_generic.inc"
namespace hsrle { void register_w48(CodecLaunch *t) { register_width(t); } }
