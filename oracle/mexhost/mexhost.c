/* Bodies of the runnable MEX host declared in matrix.h / mex.h (TEST INFRASTRUCTURE).  Column-major storage throughout. */
#include <math.h>
#include <setjmp.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include "mex.h"

struct mxArray_tag {
    mxClassID cls;
    mwSize ndim;
    mwSize *dims;
    size_t numel;
    double *pr;          /* mxDOUBLE_CLASS */
    mxLogical *lg;       /* mxLOGICAL_CLASS */
    mxArray **items;     /* mxCELL_CLASS: numel; mxSTRUCT_CLASS: numel * nfields, element-major */
    int nfields;
    char **fields;
};

static void *xcalloc(size_t n, size_t s) {
    void *p = calloc(n ? n : 1, s ? s : 1);
    if (!p) { fprintf(stderr, "mexhost: out of memory\n"); abort(); }
    return p;
}

static mxArray *new_array(mxClassID cls, mwSize ndim, const mwSize *dims) {
    mxArray *a = (mxArray *)xcalloc(1, sizeof *a);
    mwSize i, nd = ndim < 2 ? 2 : ndim;
    a->cls = cls;
    a->ndim = nd;
    a->dims = (mwSize *)xcalloc(nd, sizeof(mwSize));
    a->numel = 1;
    for (i = 0; i < nd; i++) {
        a->dims[i] = i < ndim ? dims[i] : 1;
        a->numel *= a->dims[i];
    }
    return a;
}

mxArray *mxCreateNumericArray(mwSize ndim, const mwSize *dims, mxClassID classid, mxComplexity flag) {
    mxArray *a;
    if (classid != mxDOUBLE_CLASS || flag != mxREAL) return NULL;
    a = new_array(mxDOUBLE_CLASS, ndim, dims);
    a->pr = (double *)xcalloc(a->numel, sizeof(double));
    return a;
}

mxArray *mxCreateDoubleMatrix(mwSize m, mwSize n, mxComplexity flag) {
    mwSize d[2];
    d[0] = m; d[1] = n;
    return mxCreateNumericArray(2, d, mxDOUBLE_CLASS, flag);
}

mxArray *mxCreateDoubleScalar(double value) {
    mxArray *a = mxCreateDoubleMatrix(1, 1, mxREAL);
    a->pr[0] = value;
    return a;
}

mxArray *mxCreateCellArray(mwSize ndim, const mwSize *dims) {
    mxArray *a = new_array(mxCELL_CLASS, ndim, dims);
    a->items = (mxArray **)xcalloc(a->numel, sizeof(mxArray *));
    return a;
}

mxArray *mxCreateCellMatrix(mwSize m, mwSize n) {
    mwSize d[2];
    d[0] = m; d[1] = n;
    return mxCreateCellArray(2, d);
}

mxArray *mxCreateStructMatrix(mwSize m, mwSize n, int nfields, const char **fieldnames) {
    mwSize d[2];
    mxArray *a;
    int k;
    d[0] = m; d[1] = n;
    a = new_array(mxSTRUCT_CLASS, 2, d);
    a->nfields = nfields;
    a->fields = (char **)xcalloc((size_t)nfields, sizeof(char *));
    for (k = 0; k < nfields; k++) {
        a->fields[k] = (char *)xcalloc(strlen(fieldnames[k]) + 1, 1);
        strcpy(a->fields[k], fieldnames[k]);
    }
    a->items = (mxArray **)xcalloc(a->numel * (size_t)nfields, sizeof(mxArray *));
    return a;
}

mxArray *mxCreateLogicalScalar(mxLogical value) {
    mwSize d[2] = {1, 1};
    mxArray *a = new_array(mxLOGICAL_CLASS, 2, d);
    a->lg = (mxLogical *)xcalloc(1, sizeof(mxLogical));
    a->lg[0] = value;
    return a;
}

mxArray *mxDuplicateArray(const mxArray *pa) {
    mxArray *a;
    size_t i, n;
    if (!pa) return NULL;
    a = new_array(pa->cls, pa->ndim, pa->dims);
    if (pa->cls == mxDOUBLE_CLASS) {
        a->pr = (double *)xcalloc(a->numel, sizeof(double));
        memcpy(a->pr, pa->pr, a->numel * sizeof(double));
    } else if (pa->cls == mxLOGICAL_CLASS) {
        a->lg = (mxLogical *)xcalloc(a->numel, sizeof(mxLogical));
        memcpy(a->lg, pa->lg, a->numel * sizeof(mxLogical));
    } else {
        int k;
        a->nfields = pa->nfields;
        if (pa->cls == mxSTRUCT_CLASS) {
            a->fields = (char **)xcalloc((size_t)pa->nfields, sizeof(char *));
            for (k = 0; k < pa->nfields; k++) {
                a->fields[k] = (char *)xcalloc(strlen(pa->fields[k]) + 1, 1);
                strcpy(a->fields[k], pa->fields[k]);
            }
        }
        n = a->numel * (size_t)(pa->cls == mxSTRUCT_CLASS ? pa->nfields : 1);
        a->items = (mxArray **)xcalloc(n, sizeof(mxArray *));
        for (i = 0; i < n; i++) a->items[i] = mxDuplicateArray(pa->items[i]);
    }
    return a;
}

void mxDestroyArray(mxArray *pa) {
    size_t i, n;
    int k;
    if (!pa) return;
    if (pa->items) {
        n = pa->numel * (size_t)(pa->cls == mxSTRUCT_CLASS ? pa->nfields : 1);
        for (i = 0; i < n; i++) mxDestroyArray(pa->items[i]);
        free(pa->items);
    }
    for (k = 0; k < pa->nfields && pa->fields; k++) free(pa->fields[k]);
    free(pa->fields);
    free(pa->pr);
    free(pa->lg);
    free(pa->dims);
    free(pa);
}

mxClassID mxGetClassID(const mxArray *pa) { return pa ? pa->cls : mxUNKNOWN_CLASS; }
bool mxIsDouble(const mxArray *pa) { return pa && pa->cls == mxDOUBLE_CLASS; }
bool mxIsCell(const mxArray *pa) { return pa && pa->cls == mxCELL_CLASS; }
bool mxIsStruct(const mxArray *pa) { return pa && pa->cls == mxSTRUCT_CLASS; }
bool mxIsLogical(const mxArray *pa) { return pa && pa->cls == mxLOGICAL_CLASS; }
bool mxIsLogicalScalar(const mxArray *pa) { return mxIsLogical(pa) && pa->numel == 1; }
bool mxIsLogicalScalarTrue(const mxArray *pa) { return mxIsLogicalScalar(pa) && pa->lg[0]; }
bool mxIsEmpty(const mxArray *pa) { return !pa || pa->numel == 0; }
size_t mxGetM(const mxArray *pa) { return pa->dims[0]; }
size_t mxGetN(const mxArray *pa) { return pa->dims[0] ? pa->numel / pa->dims[0] : (pa->ndim > 1 ? pa->dims[1] : 0); }
size_t mxGetNumberOfElements(const mxArray *pa) { return pa->numel; }
mwSize mxGetNumberOfDimensions(const mxArray *pa) { return pa->ndim; }
const mwSize *mxGetDimensions(const mxArray *pa) { return pa->dims; }
int mxGetNumberOfFields(const mxArray *pa) { return pa->cls == mxSTRUCT_CLASS ? pa->nfields : 0; }

double *mxGetPr(const mxArray *pa) { return pa->cls == mxDOUBLE_CLASS ? pa->pr : NULL; }

void *mxGetData(const mxArray *pa) {
    if (pa->cls == mxDOUBLE_CLASS) return pa->pr;
    if (pa->cls == mxLOGICAL_CLASS) return pa->lg;
    return pa->items;
}

double mxGetScalar(const mxArray *pa) {
    if (pa->numel == 0) return 0.0;
    if (pa->cls == mxDOUBLE_CLASS) return pa->pr[0];
    if (pa->cls == mxLOGICAL_CLASS) return pa->lg[0] ? 1.0 : 0.0;
    return 0.0;
}

mxLogical *mxGetLogicals(const mxArray *pa) { return pa->cls == mxLOGICAL_CLASS ? pa->lg : NULL; }

mxArray *mxGetCell(const mxArray *pa, mwIndex index) {
    if (!pa || pa->cls != mxCELL_CLASS || index >= pa->numel) return NULL;
    return pa->items[index];
}

void mxSetCell(mxArray *pa, mwIndex index, mxArray *value) {
    if (!pa || pa->cls != mxCELL_CLASS || index >= pa->numel) return;
    pa->items[index] = value;
}

int mxGetFieldNumber(const mxArray *pa, const char *fieldname) {
    int k;
    if (!pa || pa->cls != mxSTRUCT_CLASS) return -1;
    for (k = 0; k < pa->nfields; k++)
        if (strcmp(pa->fields[k], fieldname) == 0) return k;
    return -1;
}

mxArray *mxGetField(const mxArray *pa, mwIndex index, const char *fieldname) {
    int k = mxGetFieldNumber(pa, fieldname);
    if (k < 0 || index >= pa->numel) return NULL;
    return pa->items[index * (size_t)pa->nfields + (size_t)k];
}

void mxSetField(mxArray *pa, mwIndex index, const char *fieldname, mxArray *value) {
    int k = mxGetFieldNumber(pa, fieldname);
    if (k < 0 || index >= pa->numel) return;
    pa->items[index * (size_t)pa->nfields + (size_t)k] = value;
}

/* documented: the result is a copy of the property's value; NULL when there is no such property */
mxArray *mxGetProperty(const mxArray *pa, mwIndex index, const char *propname) {
    return mxDuplicateArray(mxGetField(pa, index, propname));
}

double mxGetNaN(void) { return NAN; }
double mxGetInf(void) { return INFINITY; }
double mxGetEps(void) { return 2.220446049250313e-16; }
void *mxMalloc(size_t n) { return xcalloc(n, 1); }
void *mxCalloc(size_t n, size_t size) { return xcalloc(n, size); }
void mxFree(void *ptr) { free(ptr); }

/* ---------------------------------------------------------------- MEX library */
#define WARN_CAP (1u << 16)
static char warn_log[WARN_CAP];
static size_t warn_len, warn_count;
static jmp_buf gate;
static int gate_open;
static char gate_msg[1024];

void mexWarnMsgTxt(const char *warn_msg) {
    size_t n = strlen(warn_msg);
    warn_count++;
    if (warn_len + n + 2 > WARN_CAP) return;    /* the count goes on, the text is full */
    memcpy(warn_log + warn_len, warn_msg, n);
    warn_len += n;
    warn_log[warn_len++] = '\n';
    warn_log[warn_len] = 0;
}

void mexErrMsgTxt(const char *error_msg) {
    strncpy(gate_msg, error_msg, sizeof gate_msg - 1);
    gate_msg[sizeof gate_msg - 1] = 0;
    if (gate_open) longjmp(gate, 1);
    fprintf(stderr, "mexErrMsgTxt outside ref_run: %s\n", gate_msg);
    abort();
}

int mexPrintf(const char *fmt, ...) {
    va_list ap;
    int n;
    va_start(ap, fmt);
    n = vprintf(fmt, ap);
    va_end(ap);
    return n;
}

int mexEvalString(const char *command) { (void)command; return 0; }

int mexCallMATLAB(int nlhs, mxArray *plhs[], int nrhs, mxArray *prhs[], const char *name) {
    int i;
    (void)nrhs; (void)prhs; (void)name;
    for (i = 0; i < nlhs; i++) plhs[i] = mxCreateDoubleScalar(0.0);
    return 0;
}

int ref_run(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[], char *errbuf, size_t errcap) {
    if (errbuf && errcap) errbuf[0] = 0;
    gate_msg[0] = 0;
    gate_open = 1;
    if (setjmp(gate) == 0) {
        mexFunction(nlhs, plhs, nrhs, prhs);
        gate_open = 0;
        return 0;
    }
    gate_open = 0;
    if (errbuf && errcap) {
        strncpy(errbuf, gate_msg, errcap - 1);
        errbuf[errcap - 1] = 0;
    }
    return 1;
}

const char *ref_warnings(void) { return warn_log; }
size_t ref_warning_count(void) { return warn_count; }
void ref_reset_warnings(void) { warn_len = 0; warn_count = 0; warn_log[0] = 0; }

/* ---------------------------------------------------------------- arrays to and from a file (for the stand-alone driver) */
static void put(FILE *f, const void *p, size_t n) { if (fwrite(p, 1, n, f) != n) abort(); }
static void get(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "mexhost: short file\n"); abort(); } }

static void save_rec(FILE *f, const mxArray *a) {
    int cls = a ? (int)a->cls : -1, k;
    size_t i, n, len;
    put(f, &cls, sizeof cls);
    if (!a) return;
    put(f, &a->ndim, sizeof a->ndim);
    put(f, a->dims, a->ndim * sizeof(mwSize));
    if (a->cls == mxDOUBLE_CLASS) put(f, a->pr, a->numel * sizeof(double));
    else if (a->cls == mxLOGICAL_CLASS) put(f, a->lg, a->numel * sizeof(mxLogical));
    else {
        put(f, &a->nfields, sizeof a->nfields);
        for (k = 0; k < a->nfields; k++) { len = strlen(a->fields[k]); put(f, &len, sizeof len); put(f, a->fields[k], len); }
        n = a->numel * (size_t)(a->cls == mxSTRUCT_CLASS ? a->nfields : 1);
        for (i = 0; i < n; i++) save_rec(f, a->items[i]);
    }
}

static mxArray *load_rec(FILE *f) {
    int cls, k, nfields;
    mwSize ndim, dims[8];
    size_t i, n, len;
    mxArray *a;
    get(f, &cls, sizeof cls);
    if (cls < 0) return NULL;
    get(f, &ndim, sizeof ndim);
    if (ndim > 8) abort();
    get(f, dims, ndim * sizeof(mwSize));
    if (cls == mxDOUBLE_CLASS) { a = mxCreateNumericArray(ndim, dims, mxDOUBLE_CLASS, mxREAL); get(f, a->pr, a->numel * sizeof(double)); return a; }
    if (cls == mxLOGICAL_CLASS) { a = mxCreateLogicalScalar(0); get(f, a->lg, sizeof(mxLogical)); return a; }
    get(f, &nfields, sizeof nfields);
    if (cls == mxSTRUCT_CLASS) {
        char **names = (char **)xcalloc((size_t)nfields, sizeof(char *));
        for (k = 0; k < nfields; k++) { get(f, &len, sizeof len); names[k] = (char *)xcalloc(len + 1, 1); get(f, names[k], len); }
        a = mxCreateStructMatrix(dims[0], ndim > 1 ? dims[1] : 1, nfields, (const char **)names);
        for (k = 0; k < nfields; k++) free(names[k]);
        free(names);
    } else
        a = mxCreateCellArray(ndim, dims);
    n = a->numel * (size_t)(cls == mxSTRUCT_CLASS ? nfields : 1);
    for (i = 0; i < n; i++) a->items[i] = load_rec(f);
    return a;
}

int ref_save(const mxArray *pa, const char *path) {
    FILE *f = fopen(path, "wb");
    if (!f) return 1;
    save_rec(f, pa);
    return fclose(f);
}

mxArray *ref_load(const char *path) {
    FILE *f = fopen(path, "rb");
    mxArray *a;
    if (!f) return NULL;
    a = load_rec(f);
    fclose(f);
    return a;
}
