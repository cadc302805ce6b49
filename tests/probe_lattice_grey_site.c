/* The one tone-map sample of tests/test_gpu_code_lattice.py where the HIP path is one code below the reference: the grey ramp's code 276 of
   the limited-range BT.2100 PQ 30bppYCbCr444 lattice image (Y 276, Cb = Cr = 512), Cr plane, HIP 127 / reference 128.  A grey pixel's chroma
   is 127.5 + 0.5 before truncation, up to the rounding of the three srgbOetf results: the knife edge between 127 and 128.  Same per-pixel
   pipeline as tests/probe_tonemap_site.c (four equal pixels: the 2 x 2 chroma average is exact), glibc's powf against a correctly rounded pow.
   cd tests && gcc -O2 -o /tmp/grey_site probe_lattice_grey_site.c -lm && /tmp/grey_site     (tests/test_code_lattice.py runs it) */
#define main probe_tonemap_site_main
#include "probe_tonemap_site.c"
#undef main
int main() {
  init_luts();
  uint16_t y[4] = {276 << 6, 276 << 6, 276 << 6, 276 << 6};
  printf("case grey 276 (Cr, hip 127 / ref 128)\n");
  run(UO_CT_PQ, UO_CG_2100, UO_CR_LIMITED, y, 512 << 6, 512 << 6);
  return 0;
}
