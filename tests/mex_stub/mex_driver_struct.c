/* mex_driver_struct.c — test infrastructure: mex_driver.c's MX / MEX stub and call grammar, with a
 * driver loop that can also print 1 x 1 STRUCT outputs (mpct_mex('eval_robust', ...) returns one).
 * mex_driver.c is compiled into this unit unchanged, its own main renamed away.
 *
 * Output: as mex_driver.c, except that a struct output k is printed as "OUT <k> T <nfields>"
 * followed by one line "FIELD <k> <name> <spec>" per field. */
#define main mex_driver_plain_main
#include "mex_driver.c"
#undef main

int main(void) {
  char word[16];
  int call = 0;
  while (scanf("%15s", word) == 1) {
    if (strcmp(word, "CALL")) {
      fprintf(stderr, "driver: expected CALL, got '%s'\n", word);
      return 3;
    }
    if (call >= MAXCALLS) return 3;
    const int nlhs = atoi(tok()), nrhs = atoi(tok());
    mxArray* prhs[16] = {0};
    mxArray* plhs[16] = {0};
    for (int k = 0; k < nrhs && k < 16; ++k) prhs[k] = parse();
    if (setjmp(g_jmp) == 0) {
      mexFunction(nlhs, plhs, nrhs, (const mxArray**)prhs);
      printf("CALL %d OK\n", call);
      for (int k = 0; k < 16; ++k) {
        const mxArray* a = plhs[k];
        if (!a) continue;
        g_out[call][k] = plhs[k];
        if (a->cls != mxSTRUCT_CLASS) {
          printf("OUT %d ", k);
          print(a);
          continue;
        }
        printf("OUT %d T %d\n", k, a->nfields);
        for (int f = 0; f < a->nfields; ++f) {
          printf("FIELD %d %s ", k, a->names[f]);
          print(a->fields[f]);
        }
      }
    } else {
      for (char* p = g_errmsg; *p; ++p)
        if (*p == '\n') *p = ' ';
      printf("CALL %d ERR %s %s\n", call, g_errid, g_errmsg);
    }
    fflush(stdout);
    free_call_allocs();
    for (int k = 0; k < nrhs && k < 16; ++k) mxDestroyArray(prhs[k]);
    ++call;
  }
  if (g_atexit) g_atexit();
  return 0;
}
