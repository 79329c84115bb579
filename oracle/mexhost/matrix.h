/*
 * A small runnable host for the part of MATLAB's C Matrix API that a plain-C MEX gateway needs (TEST INFRASTRUCTURE).
 * Written from MathWorks' published API documentation (names, argument lists and documented behaviour); bodies are in
 * mexhost.c.  Supported array kinds: real double arrays of any dimension, cell arrays, struct arrays with named fields and
 * logical scalars.  An "object" is a one-element struct: mxGetProperty looks a property up by name and, as documented,
 * hands back a copy.
 *
 * tests/mex_decls/mex.h is something else (prototypes only, for a syntax check) and stays separate.
 */
#ifndef EGDST_MEXHOST_MATRIX_H
#define EGDST_MEXHOST_MATRIX_H
#include <stddef.h>
#include <stdlib.h>
#include <stdbool.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct mxArray_tag mxArray;
typedef size_t mwSize;
typedef size_t mwIndex;
typedef bool mxLogical;
typedef enum { mxREAL = 0, mxCOMPLEX = 1 } mxComplexity;
typedef enum { mxUNKNOWN_CLASS = 0, mxCELL_CLASS = 1, mxSTRUCT_CLASS = 2, mxLOGICAL_CLASS = 3, mxDOUBLE_CLASS = 6 } mxClassID;

/* creation */
mxArray *mxCreateDoubleMatrix(mwSize m, mwSize n, mxComplexity flag);
mxArray *mxCreateDoubleScalar(double value);
mxArray *mxCreateNumericArray(mwSize ndim, const mwSize *dims, mxClassID classid, mxComplexity flag);
mxArray *mxCreateCellArray(mwSize ndim, const mwSize *dims);
mxArray *mxCreateCellMatrix(mwSize m, mwSize n);
mxArray *mxCreateStructMatrix(mwSize m, mwSize n, int nfields, const char **fieldnames);
mxArray *mxCreateLogicalScalar(mxLogical value);
mxArray *mxDuplicateArray(const mxArray *pa);
void mxDestroyArray(mxArray *pa);

/* inspection */
mxClassID mxGetClassID(const mxArray *pa);
bool mxIsDouble(const mxArray *pa);
bool mxIsCell(const mxArray *pa);
bool mxIsStruct(const mxArray *pa);
bool mxIsLogical(const mxArray *pa);
bool mxIsLogicalScalar(const mxArray *pa);
bool mxIsLogicalScalarTrue(const mxArray *pa);
bool mxIsEmpty(const mxArray *pa);
size_t mxGetM(const mxArray *pa);
size_t mxGetN(const mxArray *pa);
size_t mxGetNumberOfElements(const mxArray *pa);
mwSize mxGetNumberOfDimensions(const mxArray *pa);
const mwSize *mxGetDimensions(const mxArray *pa);
int mxGetNumberOfFields(const mxArray *pa);

/* data */
double *mxGetPr(const mxArray *pa);
void *mxGetData(const mxArray *pa);
double mxGetScalar(const mxArray *pa);
mxLogical *mxGetLogicals(const mxArray *pa);

/* containers */
mxArray *mxGetCell(const mxArray *pa, mwIndex index);
void mxSetCell(mxArray *pa, mwIndex index, mxArray *value);
mxArray *mxGetField(const mxArray *pa, mwIndex index, const char *fieldname);
void mxSetField(mxArray *pa, mwIndex index, const char *fieldname, mxArray *value);
int mxGetFieldNumber(const mxArray *pa, const char *fieldname);
mxArray *mxGetProperty(const mxArray *pa, mwIndex index, const char *propname);

/* constants and memory */
double mxGetNaN(void);
double mxGetInf(void);
double mxGetEps(void);
void *mxMalloc(size_t n);
void *mxCalloc(size_t n, size_t size);
void mxFree(void *ptr);

#ifdef __cplusplus
}
#endif
#endif
