"""`python train_retriever.py --do_predict ...` -- the reference's retrieval/train_retriever.py evaluation command line."""
from proqa_amd.train_retriever import main

if __name__ == "__main__":
    main()
